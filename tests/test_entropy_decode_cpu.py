"""CPU: the host half of entropy decoding on the GPU -- the pre-pass (dj_jpeg_scan_segments) finds the restart intervals of
eligible files and refuses every other file with a reason; the statement (data/entropy_decode.py) equals the host reader
byte for byte on every valid case and stays within its bounds on corrupted ones; the plan, the fallback, the switches, the
tool and the library's exports.  No tolerance anywhere: every comparison is equality."""
import ctypes
import importlib.util
import io
import os
import subprocess

import numpy as np
import pytest

import entropy_cases as E
import jpeg_pixels_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def reader():
    return E.reader()


@pytest.fixture(scope="module")
def ci():
    from jpeg_detection_resnet_ssd_amd.data import coefficient_inputs
    return coefficient_inputs


@pytest.fixture(scope="module")
def ed():
    from jpeg_detection_resnet_ssd_amd.data import entropy_decode
    return entropy_decode


def _ecs_start(data):
    at = data.index(b"\xff\xda")
    return at + 2 + ((data[at + 2] << 8) | data[at + 3])


# ---- the pre-pass ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(E.valid_cases()))
def test_segments_tile_the_entropy_coded_data(name):
    data, scan = E.valid_cases()[name], E.scan(name)
    assert scan.entropy_decodable and scan.reason == ""
    n_mcus = scan.mcus[0] * scan.mcus[1]
    assert scan.n_segments == -(-n_mcus // scan.restart_interval) >= 1
    ranges = scan.ranges
    assert ranges[0, 0] == _ecs_start(data)
    for k in range(1, scan.n_segments):      # two marker bytes between neighbours, in the cyclic order
        assert ranges[k, 0] == ranges[k - 1, 1] + 2
        assert data[ranges[k - 1, 1]:ranges[k, 0]] == bytes([0xFF, 0xD0 + (k - 1) % 8])
    assert data[ranges[-1, 1]:ranges[-1, 1] + 2] == b"\xff\xd9"
    for begin, end in ranges:                 # nothing of the form FF xx inside but FF 00
        body = data[begin:end]
        assert all(body[i + 1] == 0 for i in range(len(body) - 1) if body[i] == 0xFF) and not body.endswith(b"\xff")
    gray = scan.n_components == 1
    assert scan.mcu_blocks == ([(1, 1)] if gray else {"444": [(1, 1)] * 3, "422": [(1, 2), (1, 1), (1, 1)]}.get(name[:3], [(2, 2), (1, 1), (1, 1)]))
    assert len(scan.tables) == (2 if gray else 4)


def test_a_single_interval_without_a_marker_is_eligible():
    scan = E.scan("8x8")
    assert scan.entropy_decodable and scan.n_segments == 1 and b"\xff\xdd" in E.valid_cases()["8x8"]
    assert not any(bytes([0xFF, 0xD0 + k]) in E.valid_cases()["8x8"][_ecs_start(E.valid_cases()["8x8"]):] for k in range(8))


def test_optimised_tables_are_eligible():
    assert E.scan("160x160_q95_opt_i1").entropy_decodable and E.scan("48x64_i3").entropy_decodable


def test_refusals_name_a_reason_and_never_raise(reader):
    def refused(data, word):
        scan = reader.scan_segments(data)
        assert not scan.entropy_decodable and scan.n_segments == 0 and word in scan.reason, (word, scan.reason)
    refused(E.jpeg(48, 64), "no restart interval")                                              # no DRI
    refused(E.jpeg(48, 64, progressive=True, restart_marker_blocks=1), "SOF2")                  # progressive
    refused(E.jpeg(48, 64, layout="444", restart_marker_blocks=1)[:2] + b"junk", "")            # not a JPEG past SOI
    refused(b"", "empty")
    data = E.valid_cases()["48x64_i1"]
    scan = E.scan("48x64_i1")
    m0, m1 = int(scan.ranges[0, 1]), int(scan.ranges[1, 1])
    assert data[m0:m0 + 2] == b"\xff\xd0" and data[m1:m1 + 2] == b"\xff\xd1"
    refused(data[:m0] + data[m0 + 2:], "RST1 where RST0")                                       # a marker removed
    refused(data[:m0] + b"\xff\xd0" + data[m0:], "RST0 where RST1")                             # a marker duplicated
    refused(data[:m1] + b"\xff\xd2" + data[m1 + 2:], "RST2 where RST1")                         # out of order
    last = int(scan.ranges[-1, 0]) - 2
    refused(data[:last] + data[last + 2:], "10 restart markers where 11")                       # the last one removed
    refused(data[:-2], "without an end-of-image")                                               # no EOI
    refused(data[:m1] + b"\xff\xdc" + data[m1 + 2:], "FF DC")                                   # DNL
    refused(data[:-2] + data[data.index(b"\xff\xda"):], "FF DA")                                # a second scan
    # more than one scan for the components: Pillow's progressive aside, a non-interleaved file made by hand is not needed --
    # a scan that names one of three components is refused by its count
    at = data.index(b"\xff\xda")
    one = bytearray(data)
    one[at + 4] = 1
    refused(bytes(one), "names 1 of 3 components")


def test_every_proper_prefix_is_refused(reader):
    for name in ("16x16", "gray_40x24"):
        data = E.valid_cases()[name]
        for n in range(len(data)):
            scan = reader.scan_segments(data[:n])
            assert not scan.entropy_decodable and scan.reason, (name, n)


def _device_table_decodes(table, codes):
    """Every code of a table, decoded through the device form's three steps, gives its symbol; a 16-bit pattern that starts
    with no code gives length 0."""
    lut = table[:512].view(np.uint16)
    limit, offset, symbols = table[512:576].view(np.int32), table[576:640].view(np.int32), table[640:]

    def decode(look):
        e = int(lut[look >> 8])
        if e:
            return e >> 8, e & 255
        for l in range(9, 17):
            if look < limit[l - 1]:
                return l, int(symbols[((look >> (16 - l)) + offset[l - 1]) & 255])
        return 0, None
    for (l, code), symbol in codes.items():
        for tail in (0, (1 << (16 - l)) - 1):
            assert decode((code << (16 - l)) | tail) == (l, symbol)
    assert decode(0xFFFF) == (0, None)          # libjpeg's tables never use the all-ones code


def test_device_tables_hold_the_files_codes(ed):
    for name in ("48x64_i1", "160x160_q95_opt_i1", "gray_40x24", "48x64_i3"):
        scan = E.scan(name)
        codes, selectors = ed.huffman_tables(E.valid_cases()[name])
        for c, (td, ta) in enumerate(selectors):
            _device_table_decodes(scan.tables[scan.dc_table[c]], codes[(0, td)])
            _device_table_decodes(scan.tables[scan.ac_table[c]], codes[(1, ta)])


# ---- the statement ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(E.valid_cases()))
def test_statement_equals_the_host_reader(name):
    planes, status, _ = E.statement(name)
    want = E.host_planes(E.valid_cases()[name])
    assert not status.any() and len(status) == E.scan(name).n_segments
    assert len(planes) == len(want)
    for got, w in zip(planes, want):
        assert got.dtype == np.int16 and got.shape == w.shape and np.array_equal(got, w)


def test_default_segments_are_the_files_own(ed):
    planes, status = ed.entropy_decode_host(E.valid_cases()["17x33_q10_i2"])
    assert all(np.array_equal(a, b) for a, b in zip(planes, E.statement("17x33_q10_i2")[0])) and not status.any()
    with pytest.raises(ValueError, match="no restart interval"):
        ed.entropy_decode_host(E.jpeg(16, 16))


def test_the_cases_reach_every_path():
    cov = E.coverage()
    print(cov)
    assert cov["stuffed"] >= 1                     # FF 00
    assert cov["markers_in_one_file"] > 8          # the RSTn numbering wraps
    assert cov["long_codes"] >= 1                  # a consumed code longer than 9 bits
    assert cov["zrl"] >= 1 and cov["eob"] >= 1
    assert cov["full_blocks"] >= 1                 # a block that reaches k = 63 without an end-of-block symbol
    assert cov["max_dc_category"] == 11
    assert cov["interval_does_not_divide_the_row"] and cov["last_segment_shorter"]
    assert cov["padding_blocks"] >= 1              # MCU padding decoded and dropped


def test_corrupted_segments_stay_within_bounds_and_reach_every_status():
    original, scan = E.valid_cases()[E.CORRUPTED_CASE], E.scan(E.CORRUPTED_CASE)
    valid = E.statement(E.CORRUPTED_CASE)[0]
    seen = np.zeros(5, dtype=np.int64)
    for seed in E.CORRUPTED_SEEDS:
        data = E.corrupted(seed)
        at = [i for i in range(len(data)) if data[i] != original[i]]
        assert len(at) == 1 and len(data) == len(original)
        hit = int(np.flatnonzero((scan.ranges[:, 0] <= at[0]) & (at[0] < scan.ranges[:, 1]))[0])
        planes, status = E.corrupted_statement(seed)          # returns: every loop of the statement is bounded
        assert status.min() >= 0 and status.max() <= 4
        assert not np.delete(status, hit).any()               # the other segments are unaffected
        seen += np.bincount(status, minlength=5)
        if not status.any():
            continue
        # interval 3 over rows of 4 MCUs: segment s holds MCUs 3 s .. 3 s + 2; the blocks of every other segment are the
        # valid file's
        for mcu in range(12):
            if mcu // 3 != hit:
                my, mx = divmod(mcu, 4)
                assert np.array_equal(planes[0][2 * my:2 * my + 2, 2 * mx:2 * mx + 2], valid[0][2 * my:2 * my + 2, 2 * mx:2 * mx + 2])
                assert all(np.array_equal(planes[c][my, mx], valid[c][my, mx]) for c in (1, 2))
    print("segment statuses 0..4 over %d variants: %s" % (len(E.CORRUPTED_SEEDS), seen.tolist()))
    assert (seen >= 5).all(), seen.tolist()


def test_an_error_zeroes_its_block_and_the_rest_of_its_segment(ed):
    """A segment cut to its first bytes: status 4, the blocks before the cut kept, the failing block and all later ones
    zero -- in walk order, which for luma is not raster order."""
    name = "48x64_rows1"
    data, scan = E.valid_cases()[name], E.scan(name)
    valid = E.statement(name)[0]
    import copy
    cut = copy.copy(scan)
    cut.ranges = scan.ranges.copy()
    cut.ranges[1, 1] = cut.ranges[1, 0] + (scan.ranges[1, 1] - scan.ranges[1, 0]) // 2
    planes, status = ed.entropy_decode_host(data, cut)
    assert status.tolist() == [0, 4, 0]
    walk = []                                      # (component, row, col) of MCU row 1 in decoding order
    for mx in range(4):
        walk += [(0, 2 + by, 2 * mx + bx) for by in (0, 1) for bx in (0, 1)] + [(1, 1, mx), (2, 1, mx)]
    kept = [np.array_equal(planes[c][r, k], valid[c][r, k]) and valid[c][r, k].any() for c, r, k in walk]
    zero = [not planes[c][r, k].any() for c, r, k in walk]
    first_zero = zero.index(True)
    assert 0 < first_zero < len(walk) and all(kept[:first_zero]) and all(zero[first_zero:])
    for c in range(3):                             # rows 0 and 2 of MCUs untouched
        rows = (slice(0, 2), slice(4, 6)) if c == 0 else (slice(0, 1), slice(2, 3))
        assert all(np.array_equal(planes[c][r], valid[c][r]) for r in rows)


# ---- the plan, the fallback, the switches ------------------------------------------------------------------------------------------
def test_plan_layout(ci, reader):
    files = [E.valid_cases()[n] for n in ("48x64_i5", "gray_40x24", "17x33_q10_i2")]
    emit = ci.DeviceCoefficientInputs(device_entropy=True)
    pending = emit(files, [(16, 16, 16, 16), (0, 0, 16, 16), (0, 0, 16, 16)], [True, False, False])
    plan = pending.plan
    assert type(plan) is ci.EntropyCoefficientPlan and emit.host_batches == 0
    names = ("desc", "tables", "entropy", "segments", "huffman", "bytes")
    offsets = [getattr(plan, n + "_offset") for n in names]
    assert offsets[0] == 0 and all(o % 64 == 0 for o in offsets) and offsets == sorted(offsets)
    sizes = [plan.desc.nbytes, plan.tables.nbytes, plan.entropy.nbytes, plan.segments.nbytes, plan.huffman.nbytes, sum(map(len, files))]
    assert all(offsets[k] + sizes[k] <= offsets[k + 1] for k in range(5)) and plan.nbytes == offsets[5] + sizes[5]
    scans = [reader.scan_segments(f) for f in files]
    assert plan.n_status == len(plan.segments) == sum(s.n_segments for s in scans) == 3 + 4 + 3
    assert plan.scratch_bytes == plan.coef_bytes + 4 * plan.n_status and plan.coef_bytes % 64 == 0
    assert plan.huffman.shape == (12, reader.HUFF_BYTES) and not plan.huffman[6:8].any()          # the gray file has two tables
    staging = np.full(plan.nbytes + 7, 0xA5, dtype=np.uint8)
    plan.fill(staging, pending.images, n_threads=1)
    assert (staging[plan.nbytes:] == 0xA5).all()
    edesc, segs, huff, data = plan.entropy_views(staging[:plan.nbytes])
    assert np.array_equal(edesc, plan.entropy) and np.array_equal(segs, plan.segments) and np.array_equal(huff, plan.huffman)
    assert data.tobytes() == b"".join(files)
    assert np.array_equal(plan.views(staging)[0], plan.desc)
    # records: every file's segments in order, ranges moved to where its bytes lie, MCUs tiling the file
    for i, (scan, d) in enumerate(zip(scans, plan.entropy)):
        mine = segs[d["seg_first"]:d["seg_first"] + d["n_segments"]]
        assert (mine["file"] == i).all() and np.array_equal(mine["begin"] - plan.file_offsets[i], scan.ranges[:, 0])
        assert mine["first_mcu"].tolist() == list(range(0, scan.mcus[0] * scan.mcus[1], scan.restart_interval))
        assert mine["n_mcus"].sum() == scan.mcus[0] * scan.mcus[1] == d["mcus_x"] * d["mcus_y"]
        assert d["plane_offset"][:scan.n_components].tolist() == plan.desc[i]["coef_offset"][:scan.n_components].tolist()
    assert segs["n_mcus"].tolist() == [5, 5, 2, 4, 4, 4, 3, 2, 2, 2]


def test_all_or_nothing_fallback_and_its_counter(ci):
    marked, plain = E.valid_cases()["48x64_i1"], E.jpeg(48, 64)
    emit = ci.DeviceCoefficientInputs(device_entropy=True)
    assert type(emit([marked, marked]).plan) is ci.EntropyCoefficientPlan and emit.host_batches == 0
    mixed = emit([marked, plain, marked])
    assert type(mixed.plan) is ci.CoefficientPlan and emit.host_batches == 1
    assert type(mixed.sliced(slice(0, 1)).plan) is ci.EntropyCoefficientPlan and emit.host_batches == 1      # slices do not count
    assert type(emit([plain]).plan) is ci.CoefficientPlan and emit.host_batches == 2
    off = ci.DeviceCoefficientInputs()
    assert off.device_entropy is False and type(off([marked]).plan) is ci.CoefficientPlan and off.host_batches == 0
    # the statement is the same either way
    assert all(np.array_equal(a, b) for a, b in zip(emit([marked]).numpy(), off([marked]).numpy()))


def test_failures_name_the_files(ci):
    files = [E.valid_cases()["48x64_i5"], E.valid_cases()["gray_40x24"]]
    pending = ci.DeviceCoefficientInputs(device_entropy=True)(files, [(0, 0, 16, 16)] * 2)
    pending.images[1].name = "some/where.jpg"
    status = np.zeros(pending.plan.n_status, dtype=np.int32)
    assert pending.plan.failures(status, pending.images) is None
    status[[2, 5]] = [3, 4]
    text = pending.plan.failures(status, pending.images)
    assert "file 0: segment 2: AC run past the block end" in text and "file 1 (some/where.jpg): segment 2" in text


def test_switches():
    from jpeg_detection_resnet_ssd_amd.vgg_jpeg_keras.generators import (DCTGeneratorCoefficients, coefficient_switch,
                                                                         device_entropy_switch)
    assert device_entropy_switch({}) is False and device_entropy_switch({"DJ_COEFFICIENT_INPUTS": "1"}) is False
    assert device_entropy_switch({"DJ_COEFFICIENT_INPUTS": "1", "DJ_DEVICE_ENTROPY": "1"}) is True
    assert device_entropy_switch({"DJ_COEFFICIENT_INPUTS": "1", "DJ_DEVICE_ENTROPY": "0"}) is False
    for environ in ({"DJ_DEVICE_ENTROPY": "1"}, {"DJ_DEVICE_ENTROPY": "1", "DJ_COEFFICIENT_INPUTS": "0"}):
        with pytest.raises(ValueError, match="DJ_DEVICE_ENTROPY=1 needs DJ_COEFFICIENT_INPUTS=1"):
            coefficient_switch(environ)
        with pytest.raises(ValueError, match="DJ_DEVICE_ENTROPY"):
            device_entropy_switch(environ)
    with pytest.raises(ValueError, match="DJ_DEVICE_PREP"):
        device_entropy_switch({"DJ_COEFFICIENT_INPUTS": "1", "DJ_DEVICE_ENTROPY": "1", "DJ_DEVICE_PREP": "1"})
    with pytest.raises(ValueError, match="device_entropy needs device=True"):
        DCTGeneratorCoefficients("nowhere", "nothing", device=False, device_entropy=True)


def test_generator_and_configuration_pass_the_switch_on(tmp_path, monkeypatch, ci):
    import coefficient_inputs_cases as K
    from jpeg_detection_resnet_ssd_amd.vgg_jpeg_keras import generators
    from jpeg_detection_resnet_ssd_amd.vgg_jpeg_keras.vgg_dct_configuration import VGGDCTTrainingConfiguration
    tree = K.write_tree(str(tmp_path))
    gen = generators.DCTGeneratorCoefficients(tree[0], tree[1], batch_size=3, shuffle=False, target_length=32, device_entropy=True)
    pending, _ = gen[0]
    assert type(pending.plan) is ci.CoefficientPlan and gen.host_batches == 1          # that tree has no restart intervals
    assert [im.name for im in pending.images] == tree[2][:3]
    for key in ("DJ_TRAIN_DIR", "DJ_VAL_DIR", "DJ_TEST_DIR"):
        monkeypatch.setenv(key, tree[0])
    monkeypatch.setenv("DJ_INDEX_FILE", tree[1])
    for key in ("DJ_DEVICE_PREP", "DJ_DEVICE_DECODE", "DJ_PHOTOMETRIC"):
        monkeypatch.delenv(key, raising=False)
    config = VGGDCTTrainingConfiguration(lambda classes: None, "test")
    config._batch_size, config.img_size = 2, (32, 32)
    monkeypatch.setenv("DJ_COEFFICIENT_INPUTS", "1")
    config.prepare_testing_generator()
    assert config.test_generator._emit.device_entropy is False
    monkeypatch.setenv("DJ_DEVICE_ENTROPY", "1")
    config.prepare_training_generators()
    config.prepare_testing_generator()
    assert all(g._emit.device_entropy for g in (config.train_generator, config.validation_generator, config.test_generator))
    monkeypatch.delenv("DJ_COEFFICIENT_INPUTS")
    with pytest.raises(ValueError, match="DJ_DEVICE_ENTROPY=1 needs"):
        config.prepare_testing_generator()


# ---- the tool ----------------------------------------------------------------------------------------------------------------------
def test_presize_tool_restart_options(reader, tmp_path):
    from PIL import Image
    spec = importlib.util.spec_from_file_location("presize_dataset", os.path.join(ROOT, "tools", "presize_dataset.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    src = tmp_path / "src"
    os.makedirs(str(src / "n_cat"))
    pixels = C.content("noise", 40, 70)
    Image.fromarray(pixels).save(str(src / "n_cat" / "wide.png"))

    def written(*options):
        dst = tmp_path / ("dst" + "".join(options).replace("-", "_"))
        assert tool.main([str(src), str(dst), "--side", "32", "--workers", "1"] + list(options)) == 0
        return (dst / "n_cat" / "wide.jpg").read_bytes()
    # with neither option: byte for byte what the tool wrote before it had them (its save call, restated)
    im = Image.fromarray(pixels).convert("RGB").resize((56, 32), Image.BICUBIC).crop((12, 0, 44, 32))
    buf = io.BytesIO()
    im.save(buf, "JPEG", quality=90, subsampling=2, progressive=False, optimize=False)
    plain = written()
    assert plain == buf.getvalue() and not reader.scan_segments(plain).entropy_decodable
    rows = reader.scan_segments(written("--restart-rows", "1"))
    assert rows.entropy_decodable and rows.restart_interval == 2 and rows.n_segments == 2
    mcus = reader.scan_segments(written("--restart-mcus", "3"))
    assert mcus.entropy_decodable and mcus.restart_interval == 3 and mcus.n_segments == 2
    with pytest.raises(SystemExit):
        tool.main([str(src), str(tmp_path / "both"), "--restart-rows", "1", "--restart-mcus", "4"])


# ---- the libraries -----------------------------------------------------------------------------------------------------------------
def test_libraries_export_the_entry_points_and_keep_the_abi_version(ci, reader):
    from jpeg_detection_resnet_ssd_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "dj_jpeg_entropy_decode") and "dj_jpeg_entropy_decode" in _lib.SIGNATURES
    assert lib.dj_abi_version() == _lib.ABI_VERSION == 5
    assert hasattr(reader._lib(), "dj_jpeg_scan_segments")
    assert ctypes.sizeof(_lib.JpegEntropyDesc) == ci.ENTROPY_DTYPE.itemsize == 144
    assert ctypes.sizeof(_lib.JpegEntropySeg) == ci.SEGMENT_DTYPE.itemsize == 32
    for struct, dtype in ((_lib.JpegEntropyDesc, ci.ENTROPY_DTYPE), (_lib.JpegEntropySeg, ci.SEGMENT_DTYPE)):
        for name in dtype.names:
            assert getattr(struct, name).offset == dtype.fields[name][1]
    with open(os.path.join(ROOT, "include", "dj_hip.h")) as f:
        assert "#define DJ_ABI_VERSION 5" in f.read()


def test_entry_point_refuses_bad_descriptors_on_the_host(ci):
    """Every check runs before the launch, on the host copies: the pointers are never dereferenced."""
    from jpeg_detection_resnet_ssd_amd import _lib
    lib = _lib.load()
    fake = 0x10000
    files = [E.valid_cases()["48x64_i5"], E.valid_cases()["gray_40x24"]]
    plan = ci.DeviceCoefficientInputs(device_entropy=True)(files, [(0, 0, 16, 16)] * 2).plan
    n_bytes = sum(map(len, files))

    def call(desc=None, segs=None, n_bytes=n_bytes, n_tables=8, out=fake, out_bytes=plan.coef_bytes, n_segments=None):
        desc = plan.entropy if desc is None else desc
        segs = plan.segments if segs is None else segs
        return lib.dj_jpeg_entropy_decode(fake, n_bytes, fake, desc.ctypes.data, len(desc), fake, segs.ctypes.data,
                                          len(segs) if n_segments is None else n_segments, fake, n_tables, out, out_bytes, fake, None)

    def desc(file=0, **fields):
        d = plan.entropy.copy()
        for name, value in fields.items():
            d[name][file] = value
        return d

    def segs(index, **fields):
        s = plan.segments.copy()
        for name, value in fields.items():
            s[name][index] = value
        return s
    last = len(plan.segments) - 1
    cases = [({"segs": segs(0, begin=-1)}, "leave the"), ({"segs": segs(last, end=n_bytes + 1)}, "leave the"),
             ({"segs": segs(1, begin=10, end=9)}, "leave the"), ({"n_bytes": n_bytes - 3}, "leave the"),
             ({"desc": desc(plane_capacity=[48 * 64 - 1, 768, 768])}, "exceeds its capacity"),
             ({"out_bytes": plan.coef_bytes - 64}, "leave the buffer"), ({"desc": desc(plane_offset=[8, 6144, 7680])}, "multiple of 16"),
             ({"desc": desc(plane_offset=[-16, 6144, 7680])}, "leave the buffer"),
             ({"desc": desc(dc_table=[4, 1, 1])}, "table index"), ({"desc": desc(ac_table=[0, 1, -1])}, "table index"),
             ({"desc": desc(1, table_first=7)}, "table index"), ({"n_tables": 5}, "table index"),
             ({"desc": desc(1, table_first=8)}, "first table"),
             ({"desc": desc(blocks_h=[7, 3, 3])}, "do not cover"), ({"desc": desc(blocks_w=[0, 4, 4])}, "block grid"),
             ({"desc": desc(h_blocks=[5, 1, 1])}, "blocks per MCU"), ({"desc": desc(n_components=2)}, "components"),
             ({"desc": desc(mcus_x=3)}, "do not"), ({"desc": desc(n_segments=2)}, "MCUs"),
             ({"desc": desc(1, seg_first=2)}, "do not follow"), ({"segs": segs(1, file=1)}, "names file"),
             ({"segs": segs(1, first_mcu=4)}, "do not tile"), ({"segs": segs(2, n_mcus=3)}, "do not tile"),
             ({"segs": segs(0, n_mcus=0)}, "do not tile"), ({"n_segments": last}, "do not follow"),
             ({"out": fake + 8}, "aligned")]
    for kw, word in cases:
        assert call(**kw) < 0, word
        assert word.encode() in lib.dj_last_error(), (word, lib.dj_last_error())


# ---- memory safety of the pre-pass ---------------------------------------------------------------------------------------------------
def test_scan_segments_under_address_and_undefined_sanitizers(tmp_path):
    """dj_jpeg_scan_segments over case files, all their prefixes and single-byte changes, in a sanitizer build of the
    reader driven by a stand-alone program (tests/jpeg_scan_segments_asan_harness.cpp): no report, no broken promise.
    The sanitizer never enters this process."""
    flags = ["-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    # the one reason to skip, found before any work: this toolchain cannot link a sanitizer build of an empty program
    if subprocess.run(["g++"] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("g++ cannot build with -fsanitize=address,undefined here")
    exe = str(tmp_path / "jpeg_scan_segments_asan")
    r = subprocess.run(["g++"] + flags + [os.path.join(ROOT, "tests", "jpeg_scan_segments_asan_harness.cpp"),
                                           os.path.join(ROOT, "jpeg_detection_resnet_ssd_amd", "csrc", "dj_jpeg.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    files = []
    for name in ("17x33_q10_i2", "gray_40x24", "48x64_i3"):
        path = tmp_path / (name + ".jpg")
        path.write_bytes(E.valid_cases()[name])
        files.append(str(path))
    for seed in E.CORRUPTED_SEEDS[:3]:
        path = tmp_path / ("corrupted%d.jpg" % seed)
        path.write_bytes(E.corrupted(seed))
        files.append(str(path))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe] + files[:3], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, \
        (r.stdout[-1500:], r.stderr[-3000:])
    assert r.stdout.strip().endswith("bad=0") and r.stdout.count("tried=") == 3, r.stdout[-1500:]
    # the corrupted variants are not eligible as whole files or are; either way the run is clean (their prefixes may not
    # be refused for the harness's reason, so only the sanitizers' verdict counts)
    r = subprocess.run([exe] + files[3:], capture_output=True, text=True, env=env, timeout=300)
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout[-1500:], r.stderr[-3000:])
    assert r.stdout.count("tried=") == 3, r.stdout[-1500:]
