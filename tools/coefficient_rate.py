"""Cost of one batch of 64 pre-sized files (256x256, quality 90, 4:2:0) on its way to the classifier's DCT inputs at
224x224, three ways, in one run:

  (a) what a user has today: DCTGeneratorJPEG2DCT(device_prep=True, device_decode=True) -- entropy decode on 16 host
      threads, then dj_jpeg_pixels, dj_image_prep and dj_rgb_to_dct.  The batch from the generator (`gen[0]`: bytes, headers,
      draws, plan) plus `emit_into`; `emit_into` alone; the staging blob's bytes; its upload from pinned memory; the
      kernels by device events
  (b) the host coefficient path: `emit_dct_inputs(None, jpeg_bytes=...)` (decode_batch on 16 threads, de-quantised on the
      host) plus the float32 upload.  It has no window: it emits the whole 256x256 grids
  (c) the files' own coefficients: DCTGeneratorCoefficients(device=True) -- entropy decode on 16 host threads, then
      dj_jpeg_dct_inputs.  The same breakdown as (a), the kernel alone over 50 launches back to back, and its bytes moved
      (2 read and 4 written per coefficient, plus tables and descriptors) over that time
  (d) the same, entropy-decoded on the GPU: the same 64 images written with one restart interval per MCU row
      (`restart_marker_rows=1`) and fed by DCTGeneratorCoefficients(device=True, device_entropy=True) -- the files' bytes go
      up, dj_jpeg_entropy_decode makes the raw planes in device scratch, dj_jpeg_dct_inputs reads them.  Beside it, in
      the same session, (c) on those same restart-interval files with 16 host threads and with 1, which is the
      yardstick; (d)'s outputs are asserted equal to (c)'s.  `emit_into`, fill, bytes uploaded, the entropy kernel by
      events and over 50 launches back to back, and what the markers add to the files; then all of it again for
      `restart_marker_blocks=4` (four times the segments, more marker bytes)
  (e) the ordinary files of (c), which carry no restart intervals, entropy-decoded on the GPU by chunks:
      DCTGeneratorCoefficients(device=True, device_entropy=True, unmarked=True, chunk_bytes=...) for chunks of 64, 128, 256
      and 512 bytes -- `emit_into`, bytes uploaded, dj_jpeg_entropy_decode_chunked by events over 50 launches back to
      back, the median synchronisation rounds per file -- beside (c) of the same run, the yardstick; outputs asserted equal

    python tools/coefficient_rate.py [--reps 20]

(a) and (b) run code that does not depend on (c) and are the yardsticks.  Medians over `reps` with (min, max) after
warm-up; every timed window ends in a device synchronise.  Needs PIL to write the files.  Prints a markdown table and
one JSON line."""
import argparse
import io
import json
import os
import random
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from jpeg_detection_resnet_ssd_amd import kernels
from jpeg_detection_resnet_ssd_amd.data import jpeg_dct

T, SIDE, B, THREADS = 224, 256, 64, 16


def median_ms(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out), max(out)


def event_ms(fn, reps, launches=1):
    """Device time of `launches` calls of `fn` back to back, per call."""
    for _ in range(5):
        fn()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) / launches)
    return statistics.median(times), min(times), max(times)


def write_tree(root, rng, **save):
    """64 files of 256x256 in one class directory: smooth content plus noise, saved at quality 90 (PIL's 4:2:0); `save`:
    further arguments of PIL's JPEG writer (the restart interval)."""
    from PIL import Image
    directory = os.path.join(root, "train", "n_all")
    os.makedirs(directory)
    files = []
    yy, xx = np.mgrid[0:SIDE, 0:SIDE]
    for i in range(B):
        img = np.stack([127 + 100 * np.sin(xx / (11.0 + c + i % 7) + c) * np.cos(yy / (8.0 + 2 * c)) for c in range(3)], axis=-1)
        buf = io.BytesIO()
        Image.fromarray(np.clip(img + rng.normal(0, 15, img.shape), 0, 255).astype(np.uint8)).save(buf, "JPEG", quality=90, **save)
        files.append(buf.getvalue())
        with open(os.path.join(directory, "img%03d.jpg" % i), "wb") as f:
            f.write(files[-1])
    index_file = os.path.join(root, "index.json")
    with open(index_file, "w") as f:
        json.dump({"0": ["n_all", "all"]}, f)
    return os.path.join(root, "train"), index_file, files


def staged(plan, images, dev):
    staging = torch.empty(plan.nbytes, dtype=torch.uint8).pin_memory()
    plan.fill(staging.numpy(), images, THREADS)
    return staging, staging.to(dev)


def generator_rows(res, key, gen, bufs, reps):
    def batch():
        random.seed(1)
        return gen[0][0]
    res[key + "_batch_and_emit_ms"] = median_ms(lambda: batch().emit_into(bufs), reps)
    pending = batch()
    res[key + "_generator_ms"] = median_ms(batch, reps)
    res[key + "_emit_only_ms"] = median_ms(lambda: pending.emit_into(bufs), reps)
    res[key + "_blob_MB"] = pending.plan.nbytes / 1e6
    return pending


def entropy_rows(res, key, root, plain_bytes, bufs, reps, dev, **restart):
    """Rows (c) and (d) on the 64 images written with the restart interval `restart`, keys prefixed `key`."""
    from jpeg_detection_resnet_ssd_amd.vgg_jpeg_keras.generators import DCTGeneratorCoefficients
    directory, index_file, files = write_tree(os.path.join(root, key), np.random.default_rng(0), **restart)
    res[key + "_files_MB"] = sum(len(f) for f in files) / 1e6
    res[key + "_file_growth_percent"] = 100.0 * (sum(len(f) for f in files) / plain_bytes - 1.0)

    def generator(**kw):
        return DCTGeneratorCoefficients(directory, index_file, batch_size=B, shuffle=False, target_length=T, device=True, **kw)
    # (c) on these files: host entropy decoding on 16 threads and on 1
    for name, threads in (("c16", THREADS), ("c1", 1)):
        pending = generator_rows(res, key + "_" + name, generator(decode_threads=threads), bufs, reps)
        staging = torch.empty(pending.plan.nbytes, dtype=torch.uint8).pin_memory()
        res[key + "_" + name + "_fill_ms"] = median_ms(lambda: pending.plan.fill(staging.numpy(), pending.images, threads), reps)
    pending.emit_into(bufs)
    torch.cuda.synchronize()
    want = [b.clone() for b in bufs]
    # (d) entropy decoding on the GPU
    gen_d = generator(decode_threads=THREADS, device_entropy=True)
    pending_d = generator_rows(res, key + "_d", gen_d, bufs, reps)
    gen_d.check_inputs()
    assert gen_d.host_batches == 0, "every batch must take the device path"
    res[key + "_d_equals_c"] = all(bool((b == w).all()) for b, w in zip(bufs, want))
    assert res[key + "_d_equals_c"], "device_entropy=True and the host reader disagree"
    plan = pending_d.plan
    res[key + "_segments"] = plan.n_status
    staging, blob = staged(plan, pending_d.images, dev)
    host = staging.numpy()
    res[key + "_d_fill_ms"] = median_ms(lambda: plan.fill(host, pending_d.images), reps)
    res[key + "_d_upload_ms"] = median_ms(lambda: blob.copy_(staging, non_blocking=True), reps)
    scratch = torch.empty(plan.scratch_bytes, dtype=torch.uint8, device=dev)
    edesc_h, segs_h, huff_h, _ = plan.entropy_views(host)
    edesc_d, segs_d, huff_d, bytes_d = plan.entropy_views(blob)

    def entropy():
        kernels.jpeg_entropy_decode(bytes_d, edesc_d, edesc_h, segs_d, segs_h, huff_d, huff_h, scratch[:plan.coef_bytes],
                                    plan.status_view(scratch))
    res[key + "_d_entropy_kernel_ms"] = event_ms(entropy, max(50, reps))
    res[key + "_d_entropy_kernel_50_back_to_back_ms"] = event_ms(entropy, reps, launches=50)
    res[key + "_d_both_kernels_ms"] = event_ms(lambda: plan.launch(host, blob, bufs, scratch), max(50, reps))
    torch.cuda.synchronize()
    assert not plan.status_view(scratch).any().item()


CHUNK_SIZES = (64, 128, 256, 512)


def unmarked_rows(res, directory, index_file, bufs, reps, dev):
    """Row (e): the plain files through the chunked plan at every chunk size of CHUNK_SIZES; (c) was measured on them."""
    from jpeg_detection_resnet_ssd_amd.data.coefficient_inputs import ChunkedEntropyCoefficientPlan
    from jpeg_detection_resnet_ssd_amd.vgg_jpeg_keras.generators import DCTGeneratorCoefficients
    want = None
    for chunk_bytes in CHUNK_SIZES:
        key = "e%d" % chunk_bytes
        gen = DCTGeneratorCoefficients(directory, index_file, batch_size=B, shuffle=False, target_length=T, device=True,
                                       decode_threads=THREADS, device_entropy=True, unmarked=True, chunk_bytes=chunk_bytes)
        pending = generator_rows(res, key, gen, bufs, reps)
        gen.check_inputs()
        plan = pending.plan
        assert gen.host_batches == 0 and type(plan) is ChunkedEntropyCoefficientPlan, "every batch must take the chunked plan"
        if want is None:
            host_pending = DCTGeneratorCoefficients(directory, index_file, batch_size=B, shuffle=False, target_length=T,
                                                    device=True, decode_threads=THREADS)
            random.seed(1)
            want = [torch.empty_like(b) for b in bufs]
            host_pending[0][0].emit_into(want)
            torch.cuda.synchronize()
        res[key + "_equals_c"] = all(bool((b == w).all()) for b, w in zip(bufs, want))
        assert res[key + "_equals_c"], "the chunked plan and the host reader disagree"
        res[key + "_chunks"] = plan.n_chunks
        staging, blob = staged(plan, pending.images, dev)
        host = staging.numpy()
        res[key + "_fill_ms"] = median_ms(lambda: plan.fill(host, pending.images), reps)
        res[key + "_upload_ms"] = median_ms(lambda: blob.copy_(staging, non_blocking=True), reps)
        scratch = torch.empty(plan.scratch_bytes, dtype=torch.uint8, device=dev)
        rounds = torch.zeros(plan.n_status, dtype=torch.int32, device=dev)
        edesc_h, segs_h, huff_h, _ = plan.entropy_views(host)
        edesc_d, segs_d, huff_d, bytes_d = plan.entropy_views(blob)

        def entropy():
            kernels.jpeg_entropy_decode_chunked(bytes_d, edesc_d, edesc_h, segs_d, segs_h, huff_d, huff_h, scratch[:plan.coef_bytes],
                                                plan.status_view(scratch), chunk_bytes,
                                                scratch[plan.work_offset:plan.work_offset + plan.work_bytes], rounds=rounds)
        res[key + "_entropy_kernel_ms"] = event_ms(entropy, max(50, reps))
        res[key + "_entropy_kernel_50_back_to_back_ms"] = event_ms(entropy, reps, launches=50)
        res[key + "_both_kernels_ms"] = event_ms(lambda: plan.launch(host, blob, bufs, scratch), max(50, reps))
        torch.cuda.synchronize()
        assert not plan.status_view(scratch).any().item()
        per_file = rounds.cpu().numpy()
        res[key + "_rounds_median"], res[key + "_rounds_max"] = float(np.median(per_file)), int(per_file.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "coefficient_rate.py measures on the GPU"
    from jpeg_detection_resnet_ssd_amd.vgg_jpeg_keras.generators import DCTGeneratorCoefficients, DCTGeneratorJPEG2DCT
    dev = torch.device("cuda:0")
    reps = args.reps
    res = {"batch": B, "side": SIDE, "target": T, "reps": reps, "threads": THREADS}
    bufs = [torch.empty(s, device=dev) for s in jpeg_dct.input_shapes(B, T, T)]
    with tempfile.TemporaryDirectory() as root:
        directory, index_file, files = write_tree(root, np.random.default_rng(0))
        res["files_MB"] = sum(len(f) for f in files) / 1e6

        # (a) the path a user has today
        gen_a = DCTGeneratorJPEG2DCT(directory, index_file, batch_size=B, shuffle=False, target_length=T, device_prep=True,
                                     device_decode=True, decode_threads=THREADS)
        pending = generator_rows(res, "a", gen_a, bufs, reps)
        plan = pending.plan
        assert plan.decode_items == list(range(B)), "every file of the batch must travel as coefficients"
        staging, blob = staged(plan, pending.images, dev)
        host = staging.numpy()
        res["a_fill_ms"] = median_ms(lambda: plan.fill(host, pending.images, THREADS), reps)
        res["a_upload_ms"] = median_ms(lambda: blob.copy_(staging, non_blocking=True), reps)
        pixels = torch.empty(plan.out_shape, dtype=torch.uint8, device=dev)
        scratch = torch.empty(plan.scratch_bytes, dtype=torch.uint8, device=dev)
        outs = (bufs[0], bufs[1][..., :64], bufs[1][..., 64:])

        def kernels_a():
            plan.launch(host, blob, pixels, scratch)
            kernels.rgb_to_dct(pixels, gen_a._prep.tables, outs, normalized=True)
        res["a_kernels_ms"] = event_ms(kernels_a, max(50, reps))

        # (b) the host coefficient path: whole files, de-quantised on the host, float32 upload
        whole = [torch.empty(s, device=dev) for s in jpeg_dct.input_shapes(B, SIDE, SIDE)]

        def host_path():
            for buf, arr in zip(whole, jpeg_dct.emit_dct_inputs(None, jpeg_bytes=files, n_threads=THREADS)):
                buf.copy_(torch.from_numpy(arr), non_blocking=True)
        res["b_decode_and_upload_ms"] = median_ms(host_path, reps)
        res["b_decode_ms"] = median_ms(lambda: jpeg_dct.emit_dct_inputs(None, jpeg_bytes=files, n_threads=THREADS), reps)
        res["b_upload_MB"] = sum(4 * w.numel() for w in whole) / 1e6

        # (c) the files' own coefficients
        gen_c = DCTGeneratorCoefficients(directory, index_file, batch_size=B, shuffle=False, target_length=T, device=True,
                                         decode_threads=THREADS)
        pending_c = generator_rows(res, "c", gen_c, bufs, reps)
        torch.cuda.synchronize()
        res["c_equals_statement"] = all(np.array_equal(b.cpu().numpy(), w) for b, w in zip(bufs, pending_c.numpy()))
        assert res["c_equals_statement"], "dj_jpeg_dct_inputs and the host statement disagree"
        plan_c = pending_c.plan
        staging_c, blob_c = staged(plan_c, pending_c.images, dev)
        host_c = staging_c.numpy()
        res["c_fill_ms"] = median_ms(lambda: plan_c.fill(host_c, pending_c.images, THREADS), reps)
        res["c_upload_ms"] = median_ms(lambda: blob_c.copy_(staging_c, non_blocking=True), reps)
        res["c_kernel_ms"] = event_ms(lambda: plan_c.launch(host_c, blob_c, bufs), max(50, reps))
        res["c_kernel_50_back_to_back_ms"] = event_ms(lambda: plan_c.launch(host_c, blob_c, bufs), reps, launches=50)
        coefficients = sum(b.numel() for b in bufs)
        res["c_kernel_bytes"] = 6 * coefficients + plan_c.tables.nbytes + plan_c.desc.nbytes
        res["c_kernel_GBs"] = res["c_kernel_bytes"] / res["c_kernel_50_back_to_back_ms"][0] / 1e6

        # (d) entropy decoding on the GPU, beside (c) on the same restart-interval files
        plain_bytes = sum(len(f) for f in files)
        entropy_rows(res, "rows1", root, plain_bytes, bufs, reps, dev, restart_marker_rows=1)
        entropy_rows(res, "mcus4", root, plain_bytes, bufs, reps, dev, restart_marker_blocks=4)

        # (e) the plain files by chunks
        unmarked_rows(res, directory, index_file, bufs, reps, dev)

    def cell(v):
        return "%.2f (%.2f - %.2f)" % tuple(v) if isinstance(v, tuple) else ("%.2f" % v if isinstance(v, float) else str(v))
    rows = [("files on disk to input tensors: `gen[0]` + `emit_into` (ms)", "a_batch_and_emit_ms", None, "c_batch_and_emit_ms"),
            ("generator `gen[0]` alone: bytes, headers, draws, plan (ms)", "a_generator_ms", None, "c_generator_ms"),
            ("bytes in memory to input tensors: `emit_into`; (b) decode + float32 upload (ms)", "a_emit_only_ms",
             "b_decode_and_upload_ms", "c_emit_only_ms"),
            ("entropy decode into the blob / arrays, 16 threads (ms)", "a_fill_ms", "b_decode_ms", "c_fill_ms"),
            ("bytes uploaded (MB)", "a_blob_MB", "b_upload_MB", "c_blob_MB"),
            ("upload from pinned memory (ms)", "a_upload_ms", None, "c_upload_ms"),
            ("kernels by events (ms)", "a_kernels_ms", None, "c_kernel_ms"),
            ("kernel, 50 launches back to back (ms each)", None, None, "c_kernel_50_back_to_back_ms"),
            ("kernel bytes moved over that time (GB/s)", None, None, "c_kernel_GBs")]
    print("| | (a) device_prep + device_decode | (b) host coefficients, whole file | (c) own coefficients |")
    print("|---|---|---|---|")
    for name, a, b, c in rows:
        print("| %s | %s | %s | %s |" % ((name,) + tuple("-" if k is None else cell(res[k]) for k in (a, b, c))))
    print()
    print("| restart-interval files | (c) 16 host threads | (c) 1 host thread | (d) device_entropy |")
    print("|---|---|---|---|")
    for key, label in (("rows1", "one interval per MCU row"), ("mcus4", "one interval per 4 MCUs")):
        print("| **%s**: %d segments, files %.2f MB (+%.2f %%) | | | |"
              % (label, res[key + "_segments"], res[key + "_files_MB"], res[key + "_file_growth_percent"]))
        for name, suffix in (("`gen[0]` + `emit_into` (ms)", "_batch_and_emit_ms"), ("`emit_into` (ms)", "_emit_only_ms"),
                             ("fill (ms)", "_fill_ms"), ("bytes uploaded (MB)", "_blob_MB")):
            print("| %s | %s | %s | %s |" % ((name,) + tuple(cell(res[key + "_" + col + suffix]) for col in ("c16", "c1", "d"))))
        for name, k in (("upload from pinned memory (ms)", "_d_upload_ms"), ("dj_jpeg_entropy_decode by events (ms)", "_d_entropy_kernel_ms"),
                        ("dj_jpeg_entropy_decode, 50 launches back to back (ms each)", "_d_entropy_kernel_50_back_to_back_ms"),
                        ("both kernels by events (ms)", "_d_both_kernels_ms")):
            print("| %s | - | - | %s |" % (name, cell(res[key + k])))
    print()
    print("| files without restart intervals (%.2f MB) | (c) 16 host threads | %s |"
          % (res["files_MB"], " | ".join("(e) chunks of %d" % n for n in CHUNK_SIZES)))
    print("|---|---|%s" % ("---|" * len(CHUNK_SIZES)))
    for name, c, suffix in (("`gen[0]` + `emit_into` (ms)", "c_batch_and_emit_ms", "_batch_and_emit_ms"),
                            ("`emit_into` (ms)", "c_emit_only_ms", "_emit_only_ms"), ("fill (ms)", "c_fill_ms", "_fill_ms"),
                            ("bytes uploaded (MB)", "c_blob_MB", "_blob_MB"), ("upload from pinned memory (ms)", "c_upload_ms", "_upload_ms"),
                            ("chunks", None, "_chunks"), ("synchronisation rounds per file, median", None, "_rounds_median"),
                            ("synchronisation rounds per file, most", None, "_rounds_max"),
                            ("dj_jpeg_entropy_decode_chunked by events (ms)", None, "_entropy_kernel_ms"),
                            ("dj_jpeg_entropy_decode_chunked, 50 launches back to back (ms each)", None,
                             "_entropy_kernel_50_back_to_back_ms"),
                            ("both kernels by events (ms)", "c_kernel_ms", "_both_kernels_ms")):
        print("| %s | %s | %s |" % (name, "-" if c is None else cell(res[c]),
                                    " | ".join(cell(res["e%d%s" % (n, suffix)]) for n in CHUNK_SIZES)))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
