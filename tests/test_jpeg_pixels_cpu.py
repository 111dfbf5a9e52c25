"""CPU: the host statement of JPEG pixel reconstruction (data/jpeg_pixels.py) equals Pillow byte for byte; the reader's
decode verdict and batch call (include/dj_jpeg_decode.h); the staging plan with `CoefficientImage` items; the generator's
`device_decode` switch.  No tolerance anywhere: every comparison is equality."""
import io
import os
import subprocess

import numpy as np
import pytest

import jpeg_pixels_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (layout, (width, height)) at which the triangle filter on a narrow chroma component gives other bytes than Pillow
EXPECTED_DIFFERS = {("420", (1, 5)), ("420", (2, 5)), ("420", (3, 4)), ("420", (4, 3)), ("420", (2, 9)), ("420", (2, 3)),
                    ("420", (3, 2)), ("422", (3, 4)), ("422", (4, 3)), ("422", (3, 2))}


@pytest.fixture(scope="module")
def jp():
    from jpeg_detection_resnet_ssd_amd import _build
    _build.build_jpeg_library()
    from jpeg_detection_resnet_ssd_amd.data import jpeg_pixels
    return jpeg_pixels


@pytest.fixture(scope="module")
def reader(jp):
    from jpeg_detection_resnet_ssd_amd.jpeg2dct import numpy as reader
    return reader


# ---- the statement -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", C.LAYOUTS)
def test_statement_equals_pillow(jp, layout):
    """Every quality, content and size of the case table, in this sampling layout."""
    n = 0
    for size in C.SIZES:
        for quality in C.QUALITIES:
            for kind in C.CONTENTS:
                data = C.jpeg_case(layout, quality, kind, size)
                assert jp.decodable(data)
                got = jp.jpeg_pixels_host(data)
                assert got.dtype == np.uint8 and got.shape == (size[1], size[0], 3)
                assert np.array_equal(got, C.pillow_pixels(data)), (layout, quality, kind, size)
                n += 1
    assert n == len(C.SIZES) * len(C.QUALITIES) * len(C.CONTENTS)


@pytest.mark.parametrize("layout", C.LAYOUTS)
def test_statement_equals_pillow_with_optimised_tables(jp, layout):
    for size in C.SIZES[:-1]:
        for quality in (10, 90):
            data = C.jpeg_case(layout, quality, "noise", size, optimize=True)
            assert np.array_equal(jp.jpeg_pixels_host(data), C.pillow_pixels(data)), (layout, quality, size)


def _with_triangle_filter_everywhere(jp, data):
    """The statement with libjpeg's rule taken out: the triangle filter whatever the component's width."""
    info = jp.CoefficientImage(data).info.base
    h, v, height, width = info.h_samp[0], info.v_samp[0], info.height, info.width
    planes = jp.reader.loads(data, normalized=False)
    ch, cw = -(-height // v), -(-width // h)
    luma = jp.idct_blocks(planes[0], np.array(info.quant[0][:]))[:height, :width]
    chroma = []
    for c in (1, 2):
        plane = jp.idct_blocks(planes[c], np.array(info.quant[c][:]))[:ch, :cw]
        wide = np.concatenate([plane, plane[:, -1:], plane[:, -1:]], axis=1)      # wide enough for `upsample` to filter:
        chroma.append(jp.upsample(wide, h, v, height, 2 * wide.shape[1])[:, :width])      # its columns < width see cw's edge
    return jp.ycc_to_rgb(luma, chroma[0], chroma[1])


def test_narrow_chroma_components_are_replicated_not_filtered(jp):
    """libjpeg's rule on the sizes of the case table: a chroma component 2 samples or fewer across is replicated in both
    directions.  With the triangle filter applied there as everywhere else, the result differs from Pillow at the sizes
    pinned below (saturated content, quality 90); the statement equals Pillow at all of them."""
    differs = set()
    for layout in ("420", "422"):
        for size in C.SMALL_SIZES:
            data = C.jpeg_case(layout, 90, "saturated", size)
            want = C.pillow_pixels(data)
            assert np.array_equal(jp.jpeg_pixels_host(data), want), (layout, size)
            narrow = -(-size[0] // 2) <= 2
            filtered = _with_triangle_filter_everywhere(jp, data)
            if not narrow:
                assert np.array_equal(filtered, want), (layout, size)      # the helper is the statement where the rule is moot
            elif not np.array_equal(filtered, want):
                differs.add((layout, size))
    assert differs == EXPECTED_DIFFERS, sorted(differs)


def test_statement_equals_pillow_on_the_stored_files(jp):
    files = C.golden_jpegs()
    assert len(files) >= 9
    for name, data in files.items():
        if name == "progressive":
            assert not jp.decodable(data)
            with pytest.raises(ValueError):
                jp.jpeg_pixels_host(data)
            continue
        assert jp.decodable(data), name
        assert np.array_equal(jp.jpeg_pixels_host(data), C.pillow_pixels(data)), name


@pytest.mark.parametrize("layout", C.LAYOUTS)
def test_rect_equals_slicing_the_full_result(jp, layout):
    for size in C.SIZES:
        data = C.jpeg_case(layout, 75, "noise", size)
        full = jp.jpeg_pixels_host(data)
        image = jp.CoefficientImage(data)
        assert image.shape == full.shape
        for ya, yb, xa, xb in C.rectangles(size[1], size[0]):
            got = image.pixels((ya, yb, xa, xb))
            assert got.flags.c_contiguous and np.array_equal(got, full[ya:yb, xa:xb]), (size, (ya, yb, xa, xb))
    with pytest.raises(ValueError):
        jp.jpeg_pixels_host(data, (0, size[1] + 1, 0, 1))


# ---- the verdict -------------------------------------------------------------------------------------------------------
def _pil_bytes(pixels, mode="RGB", **kwargs):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(pixels).convert(mode).save(buf, "JPEG", **kwargs)
    return buf.getvalue()


def test_verdict(jp, reader):
    px = C.content("noise", 20, 28)
    for data, want in ((_pil_bytes(px), True), (_pil_bytes(px, "L"), True), (_pil_bytes(px, progressive=True), False),
                       (_pil_bytes(px, "CMYK"), False), (_pil_bytes(px, subsampling=1), True), (b"no jpeg", False),
                       (_pil_bytes(px)[:40], False)):
        assert jp.decodable(data) is want
    info = reader.decode_info(_pil_bytes(px))
    assert (info.base.width, info.base.height, info.base.n_components, info.precision) == (28, 20, 3, 8)
    assert info.saw_jfif == 1 and info.saw_adobe == 0 and list(info.component_id[:3]) == [1, 2, 3]
    info = reader.decode_info(_pil_bytes(px, "CMYK"))
    assert info.base.n_components == 4 and info.saw_adobe == 1 and info.device_decodable == 0
    assert reader.decode_info(_pil_bytes(px, progressive=True)).base.sof == 2
    # libjpeg's colour-space rule on hand-edited headers: without JFIF, ids R, G, B mean RGB; an Adobe marker decides by
    # its transform byte
    data = bytearray(_pil_bytes(px, subsampling=0))
    at = data.index(b"JFIF\x00")
    data[at:at + 4] = b"JFXX"
    assert jp.decodable(bytes(data))                         # neither marker, ids 1 2 3: YCbCr
    sof = data.index(b"\xff\xc0")
    for k, cid in enumerate(b"RGB"):
        data[sof + 10 + 3 * k] = cid
    sos = data.index(b"\xff\xda")
    for k, cid in enumerate(b"RGB"):
        data[sos + 5 + 2 * k] = cid
    assert not jp.decodable(bytes(data))
    adobe = lambda transform: b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00" + bytes([transform])
    for transform, want in ((1, True), (0, False)):
        assert jp.decodable(bytes(data[:2]) + adobe(transform) + bytes(data[2:])) is want
    with pytest.raises(ValueError):
        jp.CoefficientImage(_pil_bytes(px, progressive=True))


def test_440_and_exotic_factors_are_not_decodable(jp):
    """4:4:0 (luma 1x2) as hand-edited sampling bytes: the verdict reads the frame header only."""
    data = bytearray(_pil_bytes(C.content("noise", 16, 16), subsampling=0))
    sof = data.index(b"\xff\xc0")
    for factors, want in ((0x11, True), (0x12, False), (0x41, False), (0x21, True), (0x22, True)):
        data[sof + 11] = factors
        assert jp.decodable(bytes(data)) is want, hex(factors)


def test_library_exports_the_declared_entry_points(reader):
    import ctypes
    import re
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dj_jpeg_decode.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(dj_jpeg_[a-z0-9_]+)\s*\(", header))
    assert declared == {"dj_jpeg_read_decode_info", "dj_jpeg_read_raw_batch"}
    lib = ctypes.CDLL(os.path.join(ROOT, "jpeg_detection_resnet_ssd_amd", "csrc", "libdj_jpeg.so"))
    assert all(hasattr(lib, name) for name in declared)
    assert ctypes.sizeof(reader.JpegDecodeInfo) == ctypes.sizeof(reader.JpegInfo) + 9 * 4


# ---- the batch reader ----------------------------------------------------------------------------------------------------
def _layout(reader, files):
    offsets, caps, end = np.zeros((len(files), 4), np.int64), np.zeros((len(files), 4), np.int64), 0
    for i, data in enumerate(files):
        b = reader.decode_info(data).base
        for c in range(b.n_components):
            offsets[i, c], caps[i, c] = end, b.blocks_h[c] * b.blocks_w[c] * 64
            end += 2 * caps[i, c]
    return offsets, caps, int(end)


def test_batch_reader_planes_equal_loads(reader):
    files = [data for name, data in C.golden_jpegs().items() if name != "progressive"]
    files += [C.jpeg_case(layout, 50, "noise", size) for layout in C.LAYOUTS for size in ((1, 1), (17, 33), (50, 31))]
    offsets, caps, nbytes = _layout(reader, files)
    for n_threads in (1, 3, 16):
        out = np.full(nbytes + 64, 0xAB, dtype=np.uint8)
        status = reader.read_raw_batch(files, out[:nbytes], offsets, caps, n_threads=n_threads)
        assert status.dtype == np.int32 and not status.any()
        assert (out[nbytes:] == 0xAB).all()
        for i, data in enumerate(files):
            n = reader.decode_info(data).base.n_components
            planes = reader.loads(data, normalized=False, channels=3 if n == 3 else 1)
            for c in range(n):
                got = out[offsets[i, c]:offsets[i, c] + 2 * caps[i, c]].view(np.int16)
                assert np.array_equal(got, planes[c].reshape(-1)), (i, c)


def test_batch_reader_fails_one_file_not_the_batch(reader):
    good = C.jpeg_case("420", 75, "noise", (37, 53))
    other = C.jpeg_case("gray", 75, "smooth", (16, 16))
    offsets, caps, nbytes = _layout(reader, [good, good, other, good])
    for cut in (len(good) // 2, len(good) - 40, 30):          # inside the scan (twice), inside the headers
        out = np.zeros(nbytes, dtype=np.uint8)
        status = reader.read_raw_batch([good, good[:cut], other, good], out, offsets, caps, n_threads=2)
        assert (status != 0).tolist() == [False, True, False, False], cut
        assert "image 1" in reader.last_error()
        for i, data in ((0, good), (2, other), (3, good)):
            planes = reader.loads(data, normalized=False, channels=3 if i != 2 else 1)
            for c, plane in enumerate(planes):
                assert np.array_equal(out[offsets[i, c]:offsets[i, c] + 2 * caps[i, c]].view(np.int16), plane.reshape(-1))


def test_batch_reader_refuses_every_truncated_file(reader):
    """Every proper prefix of a file fails, as Pillow refuses it -- those that end in 0xFF (the reader makes up an
    end-of-image marker there), those that cut the scan anywhere and the one that lacks only the end-of-image marker --
    and the complete file next to them is read.  `loads` keeps libjpeg's zero-filled tail."""
    for layout, size in (("420", (37, 53)), ("gray", (17, 9))):
        data = C.jpeg_case(layout, 90, "noise", size)
        assert any(data[k - 1] == 0xFF for k in range(data.index(b"\xff\xda") + 14, len(data) - 2))
        files = [data[:k] for k in range(1, len(data))] + [data]
        one, cap, nbytes = _layout(reader, [data])
        offsets = one + nbytes * np.arange(len(files), dtype=np.int64)[:, None] * (cap > 0)
        out = np.zeros(nbytes * len(files), dtype=np.uint8)
        status = reader.read_raw_batch(files, out, offsets, np.repeat(cap, len(files), axis=0), n_threads=8)
        assert (status[:-1] != 0).all(), np.flatnonzero(status[:-1] == 0) + 1
        assert status[-1] == 0
        reader.loads(data[:len(data) - 40], normalized=False)


def test_batch_reader_refuses_small_capacity_and_bad_offsets(reader):
    data = C.jpeg_case("420", 75, "noise", (17, 33))
    offsets, caps, nbytes = _layout(reader, [data, data])
    out = np.zeros(nbytes, dtype=np.uint8)
    short = caps.copy()
    short[1, 1] -= 1
    assert reader.read_raw_batch([data, data], out, offsets, short).tolist()[0] == 0
    assert reader.read_raw_batch([data, data], out, offsets, short).tolist()[1] != 0 and "too small" in reader.last_error()
    assert not reader.read_raw_batch([data, data], out, offsets, caps).any()
    for bad in (nbytes - 2, -2, 1, nbytes + 1024):
        moved = offsets.copy()
        moved[0, 2] = bad
        before = out.copy()
        status = reader.read_raw_batch([data, data], out, moved, caps)
        assert status[0] != 0 and status[1] == 0, bad
        assert np.array_equal(out, before)                    # the refused file wrote nothing; the other one the same planes
    with pytest.raises(ValueError):
        reader.read_raw_batch([data], out[::2], offsets[:1], caps[:1])
    with pytest.raises(ValueError):
        reader.read_raw_batch([data, data], out, offsets[:1], caps[:1])


def test_batch_reader_under_address_sanitizer(tmp_path):
    """Every prefix length of two small files, and corrupted copies, through an AddressSanitizer + UBSan build of the
    reader driven by a stand-alone program (tests/jpeg_raw_batch_asan_harness.cpp): no report, and the complete file read
    next to each candidate always comes out whole.  The sanitizer never enters this process."""
    flags = ["-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    # the one reason to skip, found before any work: this toolchain cannot link a sanitizer build of an empty program
    if subprocess.run(["g++"] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("g++ cannot build with -fsanitize=address,undefined here")
    exe = str(tmp_path / "jpeg_raw_batch_asan")
    r = subprocess.run(["g++"] + flags + [os.path.join(ROOT, "tests", "jpeg_raw_batch_asan_harness.cpp"),
                                           os.path.join(ROOT, "jpeg_detection_resnet_ssd_amd", "csrc", "dj_jpeg.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    files = []
    for name, data in (("c420", C.jpeg_case("420", 50, "noise", (17, 33))), ("gray", C.jpeg_case("gray", 50, "noise", (10, 9)))):
        path = tmp_path / (name + ".jpg")
        path.write_bytes(data)
        files.append(str(path))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe] + files, capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, \
        (r.stdout[-1500:], r.stderr[-3000:])
    assert r.stdout.strip().endswith("bad=0") and r.stdout.count("tried=") == 2, r.stdout[-1500:]


# ---- the plan ----------------------------------------------------------------------------------------------------------
GEOMETRIES = [(-3, -4, 50, 60, True, 2, (1, 2, 3)), (5, 3, 20, 11, False, 3, (0, 0, 0)), (0, 0, 16, 16, False, 0, (9, 9, 9)),
              (100, 100, 5, 5, False, 1, (7, 7, 7)), (1, 0, 3, 2, True, 4, (0, 0, 0))]


def _batch(jp):
    files = [C.jpeg_case("420", 90, "noise", (53, 37)), C.jpeg_case("422", 75, "smooth", (31, 50)),
             C.jpeg_case("444", 50, "noise", (16, 16)), C.jpeg_case("gray", 75, "noise", (33, 17)),
             C.jpeg_case("420", 90, "saturated", (2, 5))]
    coefficient = [jp.CoefficientImage(f) for f in files]
    return files, coefficient, [c.pixels() for c in coefficient]


def test_mixed_plan_layout_and_fill(jp, reader):
    from jpeg_detection_resnet_ssd_amd.data import device_staging as ds, patch_resize as pr
    files, coefficient, arrays = _batch(jp)
    mixed = [coefficient[0], arrays[1], coefficient[2], coefficient[3], coefficient[4]]
    assert ds.check_images(mixed)[0] is coefficient[0]
    plan = pr.PatchPlan(pr._plan_items(mixed), GEOMETRIES, 24, 24)
    plain = pr.PatchPlan([a.shape[:2] for a in arrays], GEOMETRIES, 24, 24)
    names = ("desc", "pool", "src", "decode", "tables", "coef")
    offsets = [getattr(plan, n + "_offset") for n in names]
    assert all(o % 64 == 0 for o in offsets) and offsets == sorted(offsets)
    # the parts both plans have do not move, the new ones lie behind them; image 3's window misses it: nothing of it is staged
    assert [getattr(plain, n + "_offset") for n in names[:3]] == offsets[:3] and plan.decode_offset >= plain.nbytes
    assert plan.decode_items == [0, 2, 4] and plan.decode.dtype == ds.DECODE_DTYPE and plan.nbytes == plan.coef_offset + plan.coef_bytes
    assert np.array_equal(plan.desc, plain.desc) and plan.src_bytes == plain.src_bytes
    assert plan.scratch_bytes > plain.scratch_bytes and (plan.decode["sample_offset"] >= plain.scratch_bytes).all()
    assert (plan.decode["sample_offset"] % 64 == 0).all() and (plan.decode["coef_offset"] % 64 == 0).all()
    staging = np.full(plan.nbytes + 64, 0xCD, dtype=np.uint8)
    plan.fill(staging, mixed, n_threads=3)
    assert (staging[plan.nbytes:] == 0xCD).all()
    src, desc, pool = plan.views(staging)
    full = np.full(plain.nbytes, 0xCD, dtype=np.uint8)
    plain.fill(full, arrays)
    d1, (ya, yb, xa, xb) = plan.desc[1], plan.rects[1]
    o, n = int(d1["src_offset"]), 3 * (xb - xa) * (yb - ya)
    assert np.array_equal(src[o:o + n], plain.views(full)[0][o:o + n])          # the array item's pixels are staged as ever
    for j, i in enumerate(plan.decode_items):                                  # the others' are left for the GPU to write
        o = int(plan.desc[i]["src_offset"])
        assert (src[o:o + 3] == 0xCD).all()
    decode, tables, coef = plan.decode_views(staging)
    assert np.array_equal(decode, plan.decode)
    for j, i in enumerate(plan.decode_items):
        n = coefficient[i].n_components
        planes = reader.loads(files[i], normalized=False, channels=3 if n == 3 else 1)
        for c in range(n):
            o = int(decode[j]["coef_offset"][c])
            assert np.array_equal(coef[o:o + planes[c].size * 2].view(np.int16), planes[c].reshape(-1))
            q = np.array(coefficient[i].info.base.quant[c][:])
            assert np.array_equal(tables[int(decode[j]["table_offset"]) + 64 * c:][:64], q)
    cut = jp.CoefficientImage(files[4])              # a file that shrank between planning and filling
    cut.data = files[4][:len(files[4]) - 30]
    with pytest.raises(ValueError) as e:
        plan.fill(staging, mixed[:4] + [cut])
    assert "[4]" in str(e.value)


def test_all_array_plan_is_the_plan_without_the_new_path(jp):
    """A batch without `CoefficientImage`s: no new part, the same bytes -- against a plan laid out by the parent's rules
    restated here (descriptors | pool | pixels | records, each at a multiple of 64) and against the whole filled blob of
    the twin built from (height, width) pairs."""
    from jpeg_detection_resnet_ssd_amd.data import patch_resize as pr
    from jpeg_detection_resnet_ssd_amd.data.ssd_photometric import PhotoParams
    _, _, arrays = _batch(jp)
    records = [PhotoParams(1 + i % 2, 0.5 * i, None, 1.1, None, (0, 1, 2)) for i in range(len(arrays))]
    for photometric in (None, records):
        plan = pr.PatchPlan(pr._plan_items(arrays), GEOMETRIES, 24, 24, photometric)
        assert plan.decode is None and not hasattr(plan, "coef_offset")
        up = lambda n: -(-n // 64) * 64
        pool_offset = up(plan.desc.nbytes)
        src_offset = up(pool_offset + plan.pool.nbytes)
        assert (plan.pool_offset, plan.src_offset) == (pool_offset, src_offset)
        end = src_offset + plan.src_bytes
        if photometric is not None:
            assert plan.photo_offset == up(end)
            end = plan.photo_offset + plan.photo.nbytes
        assert plan.nbytes == end
        assert plan.scratch_bytes == sum(up(3 * 24 * g[2]) for g in GEOMETRIES)
        a = np.zeros(plan.nbytes, dtype=np.uint8)
        plan.fill(a, arrays)
        twin = pr.PatchPlan([x.shape[:2] for x in arrays], GEOMETRIES, 24, 24, photometric)
        b = np.zeros(twin.nbytes, dtype=np.uint8)
        twin.fill(b, arrays)
        assert np.array_equal(a, b)


def test_pending_pixels_equal_for_arrays_and_their_coefficient_twins(jp):
    from jpeg_detection_resnet_ssd_amd.data import patch_resize as pr
    from jpeg_detection_resnet_ssd_amd.data.ssd_photometric import PhotoParams
    _, coefficient, arrays = _batch(jp)
    prep = pr.DevicePatchResize(24, 20)
    records = [PhotoParams(1 + i % 2, 3.0 * i, 0.9, None, 4.0, (2, 0, 1)) for i in range(len(arrays))]
    for photometric in (None, records):
        want = pr.PendingPatchInputs(prep, arrays, GEOMETRIES, photometric).pixels()
        mixed = [coefficient[0], arrays[1]] + coefficient[2:]
        for images in (coefficient, mixed):
            pending = pr.PendingPatchInputs(prep, images, GEOMETRIES, photometric)
            assert np.array_equal(pending.pixels(), want)
            assert np.array_equal(pending[1:3].pixels(), want[1:3])
            for a, b in zip(pending.numpy(), pr.PendingPatchInputs(prep, arrays, GEOMETRIES, photometric).numpy()):
                assert np.array_equal(a, b)


# ---- the generator -------------------------------------------------------------------------------------------------------
XML = """<annotation><folder>VOC2007</folder><filename>%s.jpg</filename><size><width>%d</width><height>%d</height><depth>3</depth></size>
<object><name>dog</name><pose>Left</pose><truncated>0</truncated><difficult>0</difficult>
<bndbox><xmin>%d</xmin><ymin>%d</ymin><xmax>%d</xmax><ymax>%d</ymax></bndbox></object></annotation>"""


@pytest.fixture(scope="module")
def voc_tree(tmp_path_factory):
    """Five images: three the GPU path covers (4:2:0, 4:4:4, gray), a progressive and a CMYK file that fall back."""
    root = str(tmp_path_factory.mktemp("voc"))
    for sub in ("JPEGImages", "Annotations", "ImageSets/Main"):
        os.makedirs(os.path.join(root, sub))
    items = [("000001", 60, 80, "RGB", {"quality": 95}), ("000002", 48, 64, "RGB", {"progressive": True}),
             ("000003", 75, 50, "RGB", {"subsampling": 0}), ("000004", 50, 70, "CMYK", {}), ("000005", 64, 48, "L", {})]
    for image_id, h, w, mode, kwargs in items:
        with open(os.path.join(root, "JPEGImages", image_id + ".jpg"), "wb") as f:
            f.write(_pil_bytes(C.content("smooth", h, w) // 2 + C.content("noise", h, w) // 2, mode, **kwargs))
        with open(os.path.join(root, "Annotations", image_id + ".xml"), "w") as f:
            f.write(XML % (image_id, w, h, 5, 6, w - 7, h - 9))
    with open(os.path.join(root, "ImageSets", "Main", "trainval.txt"), "w") as f:
        f.write("".join(i[0] + "\n" for i in items))
    return root


def _generator(voc_tree):
    from jpeg_detection_resnet_ssd_amd.data.voc_generator import DataGeneratorDCT
    gen = DataGeneratorDCT()
    gen.parse_xml([os.path.join(voc_tree, "JPEGImages")], [os.path.join(voc_tree, "ImageSets", "Main", "trainval.txt")],
                  [os.path.join(voc_tree, "Annotations")])
    return gen


def test_generator_switch_changes_nothing_but_how_pixels_travel(jp, voc_tree):
    from jpeg_detection_resnet_ssd_amd.data import ssd_augment as sa
    from jpeg_detection_resnet_ssd_amd.data.patch_resize import DevicePatchResize
    for chain, photometric in ((sa.SSDDataAugmentation, None), (sa.SSDDataAugmentationNoCrop, sa.SSDPhotometricDistortions())):
        for seed in (0, 1, 2):
            results = []
            for device_decode in (False, True):
                gen = _generator(voc_tree)
                np.random.seed(seed)
                g = gen.generate(batch_size=5, shuffle=True, transformations=[chain(48, 40, photometric_distortions=photometric)],
                                 returns=["processed_images", "processed_labels", "image_ids", "original_images"],
                                 device_prep=DevicePatchResize(48, 40), device_decode=device_decode)
                batches = [next(g) for _ in range(3)]                 # the second pass reshuffles
                results.append((batches, np.random.get_state()))
            (off, state_off), (on, state_on) = results
            assert all(np.array_equal(a, b) for a, b in zip(state_off[1:], state_on[1:])) and state_off[0] == state_on[0]
            for (p0, y0, ids0, orig0), (p1, y1, ids1, orig1) in zip(off, on):
                assert ids0 == ids1 and p0.geometries == p1.geometries
                assert all(np.array_equal(a, b) for a, b in zip(y0, y1))
                assert (p0.photometric is None) == (p1.photometric is None)
                if p0.photometric is not None:
                    assert p0.photometric == p1.photometric
                assert all(isinstance(a, np.ndarray) and np.array_equal(a, b) for a, b in zip(orig1, orig0))
                assert not any(isinstance(im, jp.CoefficientImage) for im in p0.images)
                kinds = {i: isinstance(im, jp.CoefficientImage) for i, im in zip(ids1, p1.images)}
                assert all(kinds[i] == (i in ("000001", "000003", "000005")) for i in ids1)      # the others fell back
                assert np.array_equal(p0.pixels(), p1.pixels())
                assert np.array_equal(p0.plan.desc, p1.plan.desc) and np.array_equal(p0.plan.pool, p1.plan.pool)
    with pytest.raises(ValueError) as e:
        next(_generator(voc_tree).generate(batch_size=2, device_decode=True))
    assert "device_prep" in str(e.value)
