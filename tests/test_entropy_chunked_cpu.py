"""CPU: the host half of entropy-decoding files WITHOUT restart intervals on the GPU -- the wider pre-pass
(dj_jpeg_scan_segments_unmarked) accepts them as one segment, repeats the other pre-pass on every file that one accepts and
refuses the rest with a reason; the contract (`entropy_decode_host` with the wider scan) equals the host reader; the model
of the parallel scheme (`chunked_decode_host`) equals the contract exactly on every case, corruption and chunk size, and
reaches every path of the scheme; the plan, the dispatch, the switches and the library's exports.  No tolerance anywhere."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import entropy_cases as E
import entropy_chunked_cases as H

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


def _chunk_sizes(ci):
    return H.CHUNK_SIZES + (ci.DEFAULT_CHUNK_BYTES,)


def _ecs_start(data):
    at = data.index(b"\xff\xda")
    return at + 2 + ((data[at + 2] << 8) | data[at + 3])


# ---- the pre-pass ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in H.cases() if not n.startswith("marked")])
def test_an_unmarked_file_is_one_segment_that_covers_the_scan(reader, name):
    data, scan = H.cases()[name], H.scan(name)
    assert b"\xff\xdd" not in data
    assert scan.entropy_decodable and scan.reason == "" and scan.n_segments == 1
    assert scan.restart_interval == scan.mcus[0] * scan.mcus[1]
    begin, end = (int(v) for v in scan.ranges[0])
    assert begin == _ecs_start(data) and data[end:] == b"\xff\xd9"
    old = reader.scan_segments(data)
    assert not old.entropy_decodable and old.reason == "no restart interval (DRI)" and old.n_segments == 0
    whole = E.host_planes(data)
    assert scan.grids == [p.shape[:2] for p in whole] and len(scan.tables) == (2 if scan.n_components == 1 else 4)


def test_a_dri_of_zero_is_no_restart_interval(reader):
    data = H.cases()["16x16"]
    at = data.index(b"\xff\xda")
    with_dri = data[:at] + b"\xff\xdd\x00\x04\x00\x00" + data[at:]
    scan, plain = reader.scan_segments(with_dri, unmarked=True), H.scan("16x16")
    assert scan.entropy_decodable and scan.n_segments == 1 and scan.restart_interval == plain.restart_interval
    assert np.array_equal(scan.ranges, plain.ranges + 6) and not reader.scan_segments(with_dri).entropy_decodable


@pytest.mark.parametrize("name", list(E.valid_cases()))
def test_what_the_other_pre_pass_accepts_comes_back_identical(reader, name):
    data = E.valid_cases()[name]
    old, new = reader.scan_segments(data), reader.scan_segments(data, unmarked=True)
    assert old.entropy_decodable and new.entropy_decodable
    for field in ("reason", "n_components", "restart_interval", "mcus", "grids", "mcu_blocks", "dc_table", "ac_table"):
        assert getattr(old, field) == getattr(new, field), field
    assert np.array_equal(old.tables4, new.tables4) and np.array_equal(old.ranges, new.ranges)
    inf_old, inf_new = reader.JpegSegmentInfo(), reader.JpegSegmentInfo()
    lib = reader._lib()
    assert lib.dj_jpeg_scan_segments(data, len(data), ctypes.byref(inf_old), None, 0) == 0
    assert lib.dj_jpeg_scan_segments_unmarked(data, len(data), ctypes.byref(inf_new), None, 0) == 0
    assert bytes(inf_old) == bytes(inf_new)


def test_refusals_name_a_reason_and_never_raise(reader):
    def refused(data, word):
        scan = reader.scan_segments(data, unmarked=True)
        assert not scan.entropy_decodable and scan.n_segments == 0 and word in scan.reason, (word, scan.reason)
    data = H.cases()["48x64_q90"]
    begin, end = (int(v) for v in H.scan("48x64_q90").ranges[0])
    middle = (begin + end) // 2
    refused(data[:middle] + b"\xff\xd0" + data[middle:], "more restart markers")                # a stray restart marker
    refused(data[:middle] + b"\xff\xdc" + data[middle:], "FF DC")                               # a stray DNL
    refused(data[:middle] + b"\xff\xff" + data[middle:], "FF FF")
    refused(data[:-2], "without an end-of-image")                                               # no EOI
    refused(data[:-1], "without an end-of-image")
    refused(data[:-2] + data[data.index(b"\xff\xda"):], "FF DA")                                # a second scan
    refused(E.jpeg(48, 64, progressive=True), "SOF2")
    refused(data[:2] + b"junk", "")
    refused(b"", "empty")
    one = bytearray(data)
    one[data.index(b"\xff\xda") + 4] = 1
    refused(bytes(one), "names 1 of 3 components")
    marked = E.valid_cases()["48x64_i1"]                                                        # the other pre-pass's refusals
    m0 = int(E.scan("48x64_i1").ranges[0, 1])
    refused(marked[:m0] + marked[m0 + 2:], "RST1 where RST0")


def test_every_proper_prefix_is_refused(reader):
    for name in ("16x16", "gray_33x47", "leftover_16x16"):
        data = H.cases()[name]
        for n in range(len(data)):
            scan = reader.scan_segments(data[:n], unmarked=True)
            assert not scan.entropy_decodable and scan.reason, (name, n)


def test_the_narrow_verdict_has_not_changed(reader):
    plain = E.jpeg(48, 64)
    assert reader.scan_segments(plain).entropy_decodable is False
    assert reader.scan_segments(plain).reason == "no restart interval (DRI)"
    assert reader.scan_segments(plain, unmarked=True).entropy_decodable is True


# ---- the contract and the model ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(H.cases()))
def test_contract_equals_the_host_reader(name):
    planes, status = H.contract(name)
    want = E.host_planes(H.cases()[name])
    assert not status.any() and len(status) == H.scan(name).n_segments and len(planes) == len(want)
    for got, w in zip(planes, want):
        assert got.dtype == np.int16 and got.shape == w.shape and np.array_equal(got, w)


def _model_equals(ed, data, scan, want, chunk_bytes, counters):
    planes, status, rounds = ed.chunked_decode_host(data, scan, chunk_bytes, counters)
    assert status.dtype == np.int32 and np.array_equal(status, want[1]), (chunk_bytes, status.tolist(), want[1].tolist())
    for got, w in zip(planes, want[0]):
        assert got.dtype == np.int16 and np.array_equal(got, w), chunk_bytes
    ranges = scan.ranges
    chunks = np.maximum(1, -(-(ranges[:, 1] - ranges[:, 0]) // chunk_bytes))
    assert (rounds >= 0).all() and (rounds <= chunks).all(), (rounds.tolist(), chunks.tolist())


@pytest.fixture(scope="module")
def counters(ed, ci):
    """The model over every case, corruption and chunk size, each compared with the contract; -> its counters, summed."""
    total = {}
    for chunk_bytes in _chunk_sizes(ci):
        for name, data in H.cases().items():
            _model_equals(ed, data, H.scan(name), H.contract(name), chunk_bytes, total)
        for seed in H.CORRUPTED_SEEDS:
            _model_equals(ed, H.corrupted(seed), H.scan(H.CORRUPTED_CASE), H.corrupted_contract(seed), chunk_bytes, total)
    return total


def test_model_equals_contract_and_reaches_every_path(counters, ed):
    assert set(counters) == set(ed.CHUNK_COUNTERS)
    for name in ("empty_chunks", "stuffed_first_byte", "entry_past_end", "speculative_errors", "late_redecodes",
                 "blocks_over_three_chunks", "segments_wider_than_a_workgroup", "leftover_errors"):
        assert counters[name] > 0, (name, counters)
    assert counters["max_rounds"] >= 2


def test_corruptions_reach_every_status():
    seen = np.bincount(np.concatenate([H.corrupted_contract(seed)[1] for seed in H.CORRUPTED_SEEDS]), minlength=5)
    assert (seen >= 1).all(), seen.tolist()


def test_the_leftover_case_is_what_it_is_built_for(ed):
    data, scan = H.cases()["leftover_16x16"], H.scan("leftover_16x16")
    begin, end = (int(v) for v in scan.ranges[0])
    assert (end - begin) % 16 == 1 and data[end - 2:end] == b"\xff\x00"
    total = {}
    planes, status, _ = ed.chunked_decode_host(data, scan, 16, total)
    assert total["stuffed_first_byte"] >= 1 and total["entry_past_end"] >= 1 and total["leftover_errors"] == 1
    assert not status.any() and all(np.array_equal(a, b) for a, b in zip(planes, H.contract("16x16")[0]))


def test_model_argument_checks(ed, reader):
    data = H.cases()["16x16"]
    for bad in (0, 8, 24, 4112, 8192):
        with pytest.raises(ValueError, match="chunk_bytes"):
            ed.chunked_decode_host(data, H.scan("16x16"), bad)
    with pytest.raises(ValueError, match="not entropy-decodable"):
        ed.chunked_decode_host(data, reader.scan_segments(data), 64)


# ---- the plan, the dispatch, the switches ------------------------------------------------------------------------------------------
def test_plan_layout(ci):
    v = H.cases()
    files = [v["48x64_q90"], v["marked_48x64_i5"], v["gray_33x47"]]
    emit = ci.DeviceCoefficientInputs(device_entropy=True, unmarked=True, chunk_bytes=64)
    pending = emit(files, [(0, 0, 16, 16)] * 3)
    plan = pending.plan
    assert type(plan) is ci.ChunkedEntropyCoefficientPlan and isinstance(plan, ci.EntropyCoefficientPlan) and emit.host_batches == 0
    assert plan.chunk_bytes == 64 and plan.n_status == len(plan.segments) == 1 + 3 + 1
    offsets = [getattr(plan, n + "_offset") for n in ("desc", "tables", "entropy", "segments", "huffman", "bytes")]
    assert offsets == sorted(offsets) and all(o % 64 == 0 for o in offsets)
    assert plan.nbytes == plan.bytes_offset + sum(map(len, files))
    counts = ci.chunk_counts(plan.segments, 64)
    assert counts.tolist() == [max(1, -(-int(e - b) // 64)) for b, e in zip(plan.segments["begin"], plan.segments["end"])]
    assert plan.segments["reserved"].tolist() == np.concatenate([[0], np.cumsum(counts)[:-1]]).tolist()
    assert plan.n_chunks == counts.sum() and plan.n_blocks == 12 * 6 + 12 * 6 + 5 * 6
    assert plan.status_offset == plan.coef_bytes and plan.work_offset % 64 == 0
    assert plan.work_offset >= plan.status_offset + 4 * plan.n_status
    assert plan.work_bytes == ci.chunked_scratch_bytes(plan.n_chunks, 3, 5, plan.n_blocks)
    assert plan.scratch_bytes == plan.work_offset + plan.work_bytes
    staging = np.full(plan.nbytes + 64, 0xA5, dtype=np.uint8)
    plan.fill(staging, pending.images)
    edesc, segs, huff, data = plan.entropy_views(staging[:plan.nbytes])
    assert np.array_equal(segs, plan.segments) and segs["reserved"][-1] > 0 and bytes(data) == b"".join(files)
    assert (staging[plan.nbytes:] == 0xA5).all()


def test_dispatch_and_counter(ci):
    v = H.cases()
    plain, marked = v["48x64_q90"], v["marked_48x64_i5"]
    filled = plain[:-2] + b"\xff" + plain[-2:]           # a fill byte in front of EOI: the host reader's, not the pre-pass's
    emit = ci.DeviceCoefficientInputs(device_entropy=True, unmarked=True)
    assert emit.unmarked is True and emit.chunk_bytes == ci.DEFAULT_CHUNK_BYTES and ci.DEFAULT_CHUNK_BYTES in (64, 128, 256, 512)
    assert type(emit([marked, marked]).plan) is ci.EntropyCoefficientPlan and emit.host_batches == 0      # the old plan is kept
    assert type(emit([plain, marked]).plan) is ci.ChunkedEntropyCoefficientPlan and emit.host_batches == 0
    assert type(emit([plain]).plan) is ci.ChunkedEntropyCoefficientPlan and emit.host_batches == 0
    mixed = emit([plain, filled])
    assert type(mixed.plan) is ci.CoefficientPlan and emit.host_batches == 1
    assert type(mixed.sliced(slice(0, 1)).plan) is ci.ChunkedEntropyCoefficientPlan and emit.host_batches == 1
    old = ci.DeviceCoefficientInputs(device_entropy=True)                                                   # unchanged without the switch
    assert old.unmarked is False and type(old([plain, marked]).plan) is ci.CoefficientPlan and old.host_batches == 1
    with pytest.raises(ValueError, match="unmarked=True needs device_entropy=True"):
        ci.DeviceCoefficientInputs(unmarked=True)
    for bad in (8, 24, 8192):
        with pytest.raises(ValueError, match="chunk_bytes"):
            ci.DeviceCoefficientInputs(device_entropy=True, unmarked=True, chunk_bytes=bad)


def test_a_segment_above_the_chunk_cap_takes_the_host_path(ci, ed, monkeypatch):
    plain = H.cases()["48x64_q90"]                                    # 2770 bytes of scan: 174 chunks of 16
    monkeypatch.setattr(ed, "MAX_CHUNKS", 100)
    emit = ci.DeviceCoefficientInputs(device_entropy=True, unmarked=True, chunk_bytes=16)
    assert type(emit([plain]).plan) is ci.CoefficientPlan and emit.host_batches == 1
    wide = ci.DeviceCoefficientInputs(device_entropy=True, unmarked=True, chunk_bytes=64)
    assert type(wide([plain]).plan) is ci.ChunkedEntropyCoefficientPlan and wide.host_batches == 0


def test_failures_name_the_file(ci):
    v = H.cases()
    pending = ci.DeviceCoefficientInputs(device_entropy=True, unmarked=True)([v["48x64_q90"], v["48x64_q10_opt"]],
                                                                            [(0, 0, 16, 16)] * 2)
    pending.images[1].name = "somewhere/b.jpg"
    assert pending.plan.failures(np.zeros(2, np.int32), pending.images) is None
    text = pending.plan.failures(np.array([0, 2], np.int32), pending.images)
    assert "file 1 (somewhere/b.jpg): segment 0: corrupt AC code" in text


def test_switches(ci):
    from jpeg_detection_resnet_ssd_amd.vgg_jpeg_keras.generators import DCTGeneratorCoefficients, unmarked_switch
    on = {"DJ_COEFFICIENT_INPUTS": "1", "DJ_DEVICE_ENTROPY": "1"}
    assert unmarked_switch({}) is False and unmarked_switch(on) is False
    assert unmarked_switch(dict(on, DJ_DEVICE_ENTROPY_UNMARKED="0")) is False
    assert unmarked_switch(dict(on, DJ_DEVICE_ENTROPY_UNMARKED="1")) is True
    for environ in ({"DJ_DEVICE_ENTROPY_UNMARKED": "1"}, {"DJ_DEVICE_ENTROPY_UNMARKED": "1", "DJ_COEFFICIENT_INPUTS": "1"},
                    {"DJ_DEVICE_ENTROPY_UNMARKED": "1", "DJ_COEFFICIENT_INPUTS": "1", "DJ_DEVICE_ENTROPY": "0"}):
        with pytest.raises(ValueError, match="DJ_DEVICE_ENTROPY_UNMARKED=1 needs DJ_DEVICE_ENTROPY=1"):
            unmarked_switch(environ)
    with pytest.raises(ValueError, match="unmarked needs device_entropy=True"):
        DCTGeneratorCoefficients("nowhere", "nothing", unmarked=True)


def test_generator_and_configuration_pass_the_switches_on(tmp_path, monkeypatch, ci):
    import coefficient_inputs_cases as K
    from jpeg_detection_resnet_ssd_amd.vgg_jpeg_keras import generators
    from jpeg_detection_resnet_ssd_amd.vgg_jpeg_keras.vgg_dct_configuration import VGGDCTTrainingConfiguration
    tree = K.write_tree(str(tmp_path))                                 # ordinary files: no restart intervals
    for cls in (generators.DCTGeneratorCoefficients, generators.DCTGeneratorCoefficientsDeconv):
        gen = cls(tree[0], tree[1], batch_size=3, shuffle=False, target_length=32, device_entropy=True, unmarked=True,
                  chunk_bytes=128)
        pending, _ = gen[0]
        assert type(pending.plan) is ci.ChunkedEntropyCoefficientPlan and pending.plan.chunk_bytes == 128 and gen.host_batches == 0
        assert gen._emit.deconv is cls.deconv
    for key in ("DJ_TRAIN_DIR", "DJ_VAL_DIR", "DJ_TEST_DIR"):
        monkeypatch.setenv(key, tree[0])
    monkeypatch.setenv("DJ_INDEX_FILE", tree[1])
    for key in ("DJ_DEVICE_PREP", "DJ_DEVICE_DECODE", "DJ_PHOTOMETRIC", "DJ_DEVICE_ENTROPY_UNMARKED"):
        monkeypatch.delenv(key, raising=False)
    config = VGGDCTTrainingConfiguration(lambda classes: None, "test")
    config._batch_size, config.img_size = 2, (32, 32)
    monkeypatch.setenv("DJ_COEFFICIENT_INPUTS", "1")
    monkeypatch.setenv("DJ_DEVICE_ENTROPY", "1")
    config.prepare_testing_generator()
    assert config.test_generator._emit.device_entropy is True and config.test_generator._emit.unmarked is False
    monkeypatch.setenv("DJ_DEVICE_ENTROPY_UNMARKED", "1")
    config.prepare_training_generators()
    config.prepare_testing_generator()
    assert all(g._emit.unmarked for g in (config.train_generator, config.validation_generator, config.test_generator))
    monkeypatch.delenv("DJ_DEVICE_ENTROPY")
    with pytest.raises(ValueError, match="DJ_DEVICE_ENTROPY_UNMARKED=1 needs"):
        config.prepare_testing_generator()


def test_resnet_configuration_passes_the_switch_on(tmp_path, monkeypatch):
    import importlib.util
    import coefficient_inputs_cases as K
    tree = K.write_tree(str(tmp_path))
    spec = importlib.util.spec_from_file_location("resnet_config_file", os.path.join(ROOT, "config", "resnet", "config_file.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    for key in ("DJ_DEVICE_PREP", "DJ_DEVICE_DECODE", "DJ_PHOTOMETRIC"):
        monkeypatch.delenv(key, raising=False)
    for key, value in (("DJ_COEFFICIENT_INPUTS", "1"), ("DJ_DEVICE_ENTROPY", "1"), ("DJ_DEVICE_ENTROPY_UNMARKED", "1")):
        monkeypatch.setenv(key, value)
    config = module.TrainingConfiguration.__new__(module.TrainingConfiguration)
    config.deconv, config._batch_size, config.img_size = False, 2, (32, 32)
    gen = config._coefficient_generator(tree[0], tree[1], training=False)
    assert gen._emit.device_entropy is True and gen._emit.unmarked is True


# ---- the libraries -------------------------------------------------------------------------------------------------------------------
def test_libraries_export_the_entry_points_and_keep_the_abi_version(reader, ci):
    from jpeg_detection_resnet_ssd_amd import _lib, kernels
    lib = _lib.load()
    for name in ("dj_jpeg_entropy_decode_chunked", "dj_jpeg_entropy_chunked_scratch_bytes"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert hasattr(kernels, "jpeg_entropy_decode_chunked")
    assert lib.dj_abi_version() == _lib.ABI_VERSION == 5
    assert hasattr(reader._lib(), "dj_jpeg_scan_segments_unmarked") and hasattr(reader._lib(), "dj_jpeg_scan_segments")
    for args in ((1, 1, 1, 1), (174, 2, 5, 144), (65536, 64, 64, 100000), (3, 7, 11, 13)):
        assert lib.dj_jpeg_entropy_chunked_scratch_bytes(*args) == ci.chunked_scratch_bytes(*args)


def test_entry_point_refuses_bad_arguments_on_the_host(ci):
    """Every check runs before the launch, on the host copies: the pointers are never dereferenced."""
    from jpeg_detection_resnet_ssd_amd import _lib
    lib = _lib.load()
    fake = 0x10000
    v = H.cases()
    files = [v["48x64_q90"], v["marked_48x64_i5"]]
    plan = ci.DeviceCoefficientInputs(device_entropy=True, unmarked=True, chunk_bytes=64)(files, [(0, 0, 16, 16)] * 2).plan
    n_bytes = sum(map(len, files))

    def call(desc=None, segs=None, chunk_bytes=64, scratch=fake, scratch_bytes=plan.work_bytes, out=fake, rounds=None):
        desc = plan.entropy if desc is None else desc
        segs = plan.segments if segs is None else segs
        return lib.dj_jpeg_entropy_decode_chunked(fake, n_bytes, fake, desc.ctypes.data, len(desc), fake, segs.ctypes.data, len(segs),
                                                  fake, 8, out, plan.coef_bytes, fake, chunk_bytes, scratch, scratch_bytes, rounds, None)

    def changed(array, index, **fields):
        copy = array.copy()
        for name, value in fields.items():
            copy[name][index] = value
        return copy
    cases = [({"chunk_bytes": 0}, "chunk_bytes"), ({"chunk_bytes": 8}, "chunk_bytes"), ({"chunk_bytes": 72}, "chunk_bytes"),
             ({"chunk_bytes": 8192}, "chunk_bytes"), ({"scratch": None}, "scratch is null"),
             ({"scratch_bytes": plan.work_bytes - 1}, "bytes of scratch"), ({"scratch_bytes": 0}, "bytes of scratch"),
             ({"chunk_bytes": 16}, "its first chunk"),                                # the records were made for chunks of 64
             ({"scratch": fake + 8}, "aligned"), ({"out": fake + 8}, "aligned"), ({"rounds": fake + 2}, "aligned"),
             ({"segs": changed(plan.segments, 1, reserved=0)}, "its first chunk"),
             ({"segs": changed(plan.segments, 0, begin=-1)}, "leave the"),
             ({"segs": changed(plan.segments, 2, n_mcus=3)}, "do not tile"),
             ({"desc": changed(plan.entropy, 0, dc_table=[4, 1, 1])}, "table index"),
             ({"desc": changed(plan.entropy, 1, plane_offset=[8, 0, 0])}, "multiple of 16")]
    for kw, word in cases:
        assert call(**kw) < 0, word
        assert word.encode() in lib.dj_last_error(), (word, lib.dj_last_error())


# ---- memory safety of the pre-pass -----------------------------------------------------------------------------------------------------
def test_scan_segments_unmarked_under_address_and_undefined_sanitizers(tmp_path):
    """dj_jpeg_scan_segments_unmarked over case files, all their prefixes and single-byte changes, in a sanitizer build of
    the reader driven by a stand-alone program (tests/jpeg_scan_segments_unmarked_asan_harness.cpp): no report, no broken
    promise.  The sanitizer never enters this process."""
    flags = ["-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    # the one reason to skip, found before any work: this toolchain cannot link a sanitizer build of an empty program
    if subprocess.run(["g++"] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("g++ cannot build with -fsanitize=address,undefined here")
    exe = str(tmp_path / "jpeg_scan_segments_unmarked_asan")
    r = subprocess.run(["g++"] + flags + [os.path.join(ROOT, "tests", "jpeg_scan_segments_unmarked_asan_harness.cpp"),
                                           os.path.join(ROOT, "jpeg_detection_resnet_ssd_amd", "csrc", "dj_jpeg.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    files = []
    for name, data in (("17x33_q10", H.cases()["17x33_q10"]), ("gray_33x47", H.cases()["gray_33x47"]),
                       ("leftover_16x16", H.cases()["leftover_16x16"]), ("marked", E.valid_cases()["17x33_q10_i2"])):
        path = tmp_path / (name + ".jpg")
        path.write_bytes(data)
        files.append(str(path))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe] + files, capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, \
        (r.stdout[-1500:], r.stderr[-3000:])
    assert r.stdout.strip().endswith("bad=0") and r.stdout.count("tried=") == 4 and "unmarked=0 " not in r.stdout, r.stdout[-1500:]
