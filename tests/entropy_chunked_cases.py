"""What tests/test_entropy_chunked_cpu.py and tests/test_entropy_chunked_gpu.py share: JPEG files WITHOUT restart intervals
written in-test (`entropy_cases.jpeg` with no restart option), one marked file, a hand-built file whose leftover bytes reach
the scheme's rare paths, the single-byte corruptions of one file, the contract's results
(`entropy_decode_host(data, scan_segments(data, unmarked=True))`, computed once, never changed) and the kernel's inputs."""
import functools

import numpy as np

import entropy_cases as E

CHUNK_SIZES = (16, 64)      # and the default, which the tests read from data/coefficient_inputs.py
KERNEL_ONLY = ("444_24x40", "422_17x33")      # not 4:2:0: no network input, the kernel alone


def with_leftover(data):
    """A valid unmarked file with bytes put behind its last block, in front of EOI: one byte if the scan's length is even,
    then FF 00 pairs until the segment's last chunk of 16 bytes is the 00 of a pair, alone.  A sequential decoder ignores
    them; by chunks they give a chunk whose first byte is a stuffed 00, a guess at the chunk's end and errors that are
    never met."""
    scan = E.reader().scan_segments(data, unmarked=True)
    begin, end = (int(v) for v in scan.ranges[0])
    pad = b"" if (end - begin) % 2 else b"\x7f"
    while (end - begin + len(pad)) % 16 != 1:
        pad += b"\xff\x00"
    return data[:end] + pad + data[end:]


@functools.lru_cache(maxsize=None)
def cases():
    """name -> bytes, in a fixed order."""
    return {
        "gray_8x8": E.jpeg(8, 8, layout="gray"),                      # one block, one chunk
        "16x16": E.jpeg(16, 16),
        "17x33_q10": E.jpeg(17, 33, 10),
        "48x64_q90": E.jpeg(48, 64, 90),
        "48x64_q10_opt": E.jpeg(48, 64, 10, optimize=True),
        "noise_q100": E.jpeg(32, 32, 100),                            # stuffed bytes, blocks of several hundred bits
        "gray_33x47": E.jpeg(33, 47, 50, layout="gray"),
        "saturated_q1": E.jpeg(40, 56, 1, "saturated"),
        "444_24x40": E.jpeg(24, 40, 75, layout="444"),
        "422_17x33": E.jpeg(17, 33, 50, layout="422"),
        "300x300_smooth_q90": E.jpeg(300, 300, 90, "smooth"),        # more chunks of 16 bytes than a workgroup has lanes
        "marked_48x64_i5": E.valid_cases()["48x64_i5"],
        "leftover_16x16": with_leftover(E.jpeg(16, 16)),
    }


@functools.lru_cache(maxsize=None)
def scan(name):
    return E.reader().scan_segments(cases()[name], unmarked=True)


def _frozen(planes, status):
    for p in planes:
        p.setflags(write=False)
    status.setflags(write=False)
    return planes, status


@functools.lru_cache(maxsize=None)
def contract(name):
    """-> (planes, status) of a case: the sequential statement's."""
    from jpeg_detection_resnet_ssd_amd.data.entropy_decode import entropy_decode_host
    return _frozen(*entropy_decode_host(cases()[name], scan(name)))


# ---- corruptions, made the way entropy_cases makes them ----------------------------------------------------------------------
CORRUPTED_CASE = "48x64_q10_opt"
CORRUPTED_SEEDS = tuple(range(60))


def corrupted(seed):
    """CORRUPTED_CASE with ONE byte of its scan changed, drawn from `seed` as `entropy_cases.corrupted` draws."""
    data = bytearray(cases()[CORRUPTED_CASE])
    rng = np.random.RandomState(1000 + seed)
    begin, end = (int(v) for v in scan(CORRUPTED_CASE).ranges[0])
    pos = begin + int(rng.randint(0, end - begin))
    old = data[pos]
    new = [int(rng.randint(0, 256)), 0xFF, 0xFE, 0x00, old ^ (1 << int(rng.randint(0, 8)))][int(rng.randint(0, 5))]
    data[pos] = new if new != old else old ^ 0x80
    return bytes(data)


@functools.lru_cache(maxsize=None)
def corrupted_contract(seed):
    from jpeg_detection_resnet_ssd_amd.data.entropy_decode import entropy_decode_host
    return _frozen(*entropy_decode_host(corrupted(seed), scan(CORRUPTED_CASE)))


# ---- the kernel's inputs ---------------------------------------------------------------------------------------------------
def kernel_batch(datas, scans, chunk_bytes, lead=48, gap=64):
    """`entropy_cases.kernel_batch` (planes at offsets that are multiples of 16 but not of 64, canaries around and
    between them) with the records' first chunks filled in, and the scratch the entry point needs -> dict."""
    from jpeg_detection_resnet_ssd_amd.data import coefficient_inputs as ci
    batch = E.kernel_batch(datas, scans, lead, gap)
    file_offsets = np.concatenate([[0], np.cumsum([len(d) for d in datas])]).astype(np.int64)
    desc, segs, tables, n_chunks, n_blocks = ci.chunked_records(scans, batch["plane_offsets"], file_offsets, chunk_bytes)
    assert np.array_equal(desc, batch["desc"]) and np.array_equal(tables, batch["tables"])
    batch.update(segs=segs, n_chunks=n_chunks, n_blocks=n_blocks, chunk_bytes=chunk_bytes,
                 scratch_bytes=ci.chunked_scratch_bytes(n_chunks, len(datas), len(segs), n_blocks))
    return batch
