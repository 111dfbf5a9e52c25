"""What tests/test_entropy_decode_cpu.py and tests/test_entropy_decode_gpu.py share: restart-interval JPEG files written
in-test with Pillow (`subsampling=2` or mode L, plus 4:4:4 and 4:2:2 for the kernel alone), the single-byte corruptions of
one of them, the statement's results (computed once, never changed) and the coverage conditions the files must meet --
asserted here through the statement's counters, so that no test can pass by never reaching a path."""
import functools
import io

import numpy as np

import jpeg_pixels_cases as C


def _save(image, **kw):
    buf = io.BytesIO()
    image.save(buf, "JPEG", **kw)
    return buf.getvalue()


def jpeg(height, width, quality=75, kind="noise", layout="420", seed=0, **kw):
    return C.write_jpeg(C.content(kind, height, width, seed=seed), layout, quality, **kw)


def checkerboard():
    """32 x 32 gray, 8 x 8 blocks alternately black and white, quality 100: DC differences of about 2040."""
    from PIL import Image
    yy, xx = np.mgrid[0:32, 0:32]
    pixels = (((yy // 8 + xx // 8) & 1) * 255).astype(np.uint8)
    return _save(Image.fromarray(pixels, "L"), quality=100, restart_marker_blocks=4)


@functools.lru_cache(maxsize=None)
def valid_cases():
    """name -> bytes of every valid file, in a fixed order (a dict keeps it)."""
    cases = {
        "8x8": jpeg(8, 8, restart_marker_rows=1),                                      # one MCU, one segment, no marker
        "16x16": jpeg(16, 16, restart_marker_blocks=1),
        "17x33_q10_i2": jpeg(17, 33, 10, restart_marker_blocks=2),                     # 2 x 3 MCUs: segments cross the rows
        "48x64_rows1": jpeg(48, 64, restart_marker_rows=1),
        "48x64_i1": jpeg(48, 64, restart_marker_blocks=1),                             # 11 markers: RST7 -> RST0
        # optimised tables leave more of the code space unused than the standard ones: corruptions reach "no code"
        "48x64_i3": jpeg(48, 64, 10, optimize=True, restart_marker_blocks=3),
        "48x64_i5": jpeg(48, 64, 90, restart_marker_blocks=5),                         # 5 + 5 + 2 MCUs
        "160x160_q95_opt_i1": jpeg(160, 160, 95, optimize=True, restart_marker_blocks=1),   # 100 segments, two waves
        "gray_40x24": jpeg(40, 24, 75, layout="gray", restart_marker_blocks=4),
        "gray_33x47_rows1": jpeg(33, 47, 50, layout="gray", restart_marker_rows=1),
        "noise_q100": jpeg(32, 32, 100, restart_marker_blocks=1),                      # stuffed FF 00, blocks without EOB
        "saturated_q1": jpeg(40, 56, 1, "saturated", restart_marker_blocks=2),         # long zero runs
        "checkerboard_q100": checkerboard(),
        "300x300_rows1": jpeg(300, 300, 90, "smooth", restart_marker_rows=1),
        "444_24x40_i2": jpeg(24, 40, 75, layout="444", restart_marker_blocks=2),       # the kernel alone: not 4:2:0
        "422_17x33_i2": jpeg(17, 33, 50, layout="422", restart_marker_blocks=2),
    }
    return cases


def reader():
    from jpeg_detection_resnet_ssd_amd.jpeg2dct import numpy as reader
    return reader


@functools.lru_cache(maxsize=None)
def scan(name):
    return reader().scan_segments(valid_cases()[name])


@functools.lru_cache(maxsize=None)
def statement(name):
    """-> (planes, status, counters) of a valid case: the statement's, computed once."""
    from jpeg_detection_resnet_ssd_amd.data.entropy_decode import entropy_decode_host
    counters = {}
    planes, status = entropy_decode_host(valid_cases()[name], scan(name), counters)
    for p in planes:
        p.setflags(write=False)
    status.setflags(write=False)
    return planes, status, counters


def host_planes(data):
    """The host reader's raw planes of a file: [(blocks_h, blocks_w, 64) int16]."""
    from jpeg_detection_resnet_ssd_amd.data.jpeg_pixels import CoefficientImage
    image = CoefficientImage(data)
    grids = image.grids()
    sizes = [bh * bw * 64 for bh, bw in grids]
    offsets, caps = np.zeros((1, 4), dtype=np.int64), np.zeros((1, 4), dtype=np.int64)
    offsets[0, :len(sizes)] = 2 * np.concatenate([[0], np.cumsum(sizes)[:-1]])
    caps[0, :len(sizes)] = sizes
    out = np.zeros(2 * sum(sizes), dtype=np.uint8)
    assert not reader().read_raw_batch([data], out, offsets, caps, n_threads=1).any(), reader().last_error()
    values = out.view(np.int16)
    return [values[o // 2:o // 2 + s].reshape(bh, bw, 64) for o, s, (bh, bw) in zip(offsets[0], sizes, grids)]


def coverage():
    """The conditions the valid files must meet between them -> {condition: value}; every one is asserted by the CPU test."""
    total = {}
    for name in valid_cases():
        for k, v in statement(name)[2].items():
            total[k] = max(total.get(k, 0), v) if k == "max_dc_category" else total.get(k, 0) + v
    s17, s5 = scan("17x33_q10_i2"), scan("48x64_i5")
    return {
        "stuffed": total["stuffed"], "long_codes": total["long_codes"], "zrl": total["zrl"], "eob": total["eob"],
        "full_blocks": total["full_blocks"], "max_dc_category": total["max_dc_category"],
        "padding_blocks": total["padding_blocks"],
        "markers_in_one_file": scan("48x64_i1").n_segments - 1,
        "interval_does_not_divide_the_row": s17.mcus[1] % s17.restart_interval != 0 and s5.mcus[1] % s5.restart_interval != 0,
        "last_segment_shorter": (s5.mcus[0] * s5.mcus[1]) % s5.restart_interval != 0,
    }


# ---- corrupted segments --------------------------------------------------------------------------------------------------
CORRUPTED_CASE = "48x64_i3"
CORRUPTED_SEEDS = tuple(range(200))


def corrupted(seed):
    """The bytes of CORRUPTED_CASE with ONE byte inside a segment changed, drawn from `seed`: the position uniformly over
    the segments' bytes, the new value one of a random byte, 0xFF, 0xFE, 0x00 and the old value with one bit flipped."""
    data = bytearray(valid_cases()[CORRUPTED_CASE])
    rng = np.random.RandomState(1000 + seed)
    ranges = scan(CORRUPTED_CASE).ranges
    lengths = ranges[:, 1] - ranges[:, 0]
    at = int(rng.randint(0, int(lengths.sum())))
    seg = int(np.searchsorted(np.cumsum(lengths), at, side="right"))
    pos = int(ranges[seg, 0] + at - (np.cumsum(lengths)[seg] - lengths[seg]))
    old = data[pos]
    new = [int(rng.randint(0, 256)), 0xFF, 0xFE, 0x00, old ^ (1 << int(rng.randint(0, 8)))][int(rng.randint(0, 5))]
    data[pos] = new if new != old else old ^ 0x80
    return bytes(data)


@functools.lru_cache(maxsize=None)
def corrupted_statement(seed):
    from jpeg_detection_resnet_ssd_amd.data.entropy_decode import entropy_decode_host
    planes, status = entropy_decode_host(corrupted(seed), scan(CORRUPTED_CASE))
    for p in planes:
        p.setflags(write=False)
    status.setflags(write=False)
    return planes, status


# ---- the kernel's inputs from files and their scans ------------------------------------------------------------------------
def kernel_batch(datas, scans, lead=48, gap=64):
    """Descriptors, records, tables and the bytes buffer of a batch, with every plane at a byte offset that is a multiple
    of 16 but not of 64 inside an output buffer that starts and ends with `lead` spare bytes (the canaries) and keeps
    `gap` spare bytes between planes (a multiple of 64: a plane is a multiple of 128 bytes, so every offset stays 48 mod
    64) -> dict."""
    from jpeg_detection_resnet_ssd_amd.data import coefficient_inputs as ci
    assert lead % 64 == 48 and gap % 64 == 0
    plane_offsets, at = [], lead
    for s in scans:
        mine = []
        for bh, bw in s.grids:
            assert at % 16 == 0 and at % 64 != 0
            mine.append(at)
            at += bh * bw * 128 + gap
        plane_offsets.append(mine + [0] * (3 - len(mine)))
    out_bytes = at - gap + lead
    file_offsets = np.concatenate([[0], np.cumsum([len(d) for d in datas])]).astype(np.int64)
    desc, segs, tables = ci.entropy_records(scans, plane_offsets, file_offsets)
    return {"desc": desc, "segs": segs, "tables": tables, "bytes": np.frombuffer(b"".join(datas), dtype=np.uint8).copy(),
            "out_bytes": out_bytes, "plane_offsets": plane_offsets, "grids": [s.grids for s in scans]}


def planes_of(batch, out):
    """The planes of every file from the output buffer's bytes -> [[(bh, bw, 64) int16]]; and the mask of the bytes that
    belong to no plane (the canaries and gaps)."""
    spare = np.ones(batch["out_bytes"], dtype=bool)
    files = []
    for offsets, grids in zip(batch["plane_offsets"], batch["grids"]):
        planes = []
        for at, (bh, bw) in zip(offsets, grids):
            n = bh * bw * 128
            planes.append(out[at:at + n].copy().view(np.int16).reshape(bh, bw, 64))
            spare[at:at + n] = False
        files.append(planes)
    return files, spare
